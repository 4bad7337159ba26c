"""The closure `als_fitter.get_jax_likelihood` returns (its docstring is the contract): float32 in and out around the batched
entries of a `conv_mode='jax'` fitter, wrapped for JAX where JAX is installed."""
from __future__ import annotations

import numpy as np


def jax_likelihood(twin, ndim, use_jax=None):
    """`log_likelihood(p)` over the `conv_mode='jax'` fitter `twin` of `ndim` parameters."""

    def host_loglike(p):
        p32 = np.asarray(p, dtype=np.float32)                        # jaxns hands float32 live points (:529-536)
        if p32.shape[-1:] != (ndim,):
            raise ValueError(f"parameter vectors must have {ndim} entries")
        rows = np.ascontiguousarray(p32.reshape(-1, ndim), dtype=np.float64)
        ll = twin.loglike_batch(rows).astype(np.float32)
        return ll.reshape(p32.shape[:-1]) if p32.ndim > 1 else ll.reshape(())[()]

    def host_grad(p):
        p32 = np.asarray(p, dtype=np.float32)
        if p32.shape[-1:] != (ndim,):
            raise ValueError(f"parameter vectors must have {ndim} entries")
        rows = np.ascontiguousarray(p32.reshape(-1, ndim), dtype=np.float64)
        ll, g = twin.loglike_grad_batch(rows)
        ll = ll.astype(np.float32)
        return (ll.reshape(p32.shape[:-1]) if p32.ndim > 1 else ll.reshape(())[()]), g.astype(np.float32).reshape(p32.shape)

    try:
        if use_jax is False:
            raise ImportError
        import jax
        import jax.numpy as jnp
    except ImportError:
        if use_jax:
            raise ImportError("JAX is not available.")
        host_loglike.fitter = twin
        host_loglike.host_grad = host_grad
        return host_loglike

    def value(p):                                                    # pragma: no cover - needs JAX
        shape = jax.ShapeDtypeStruct(p.shape[:-1], jnp.float32)
        return jax.pure_callback(lambda q: np.asarray(host_loglike(q), dtype=np.float32).reshape(q.shape[:-1]),
                                 shape, p, vmap_method="expand_dims")

    @jax.custom_vjp
    def log_likelihood(p):                                           # pragma: no cover - needs JAX
        return value(jnp.asarray(p, dtype=jnp.float32))

    def fwd(p):                                                      # pragma: no cover - needs JAX
        p = jnp.asarray(p)
        return value(p.astype(jnp.float32)), p

    def bwd(p, ct):                                                  # pragma: no cover - needs JAX
        # the callback is float32 in and out; the cotangent goes back in the primal's dtype (float64 under x64)
        p32 = p.astype(jnp.float32)
        g = jax.pure_callback(lambda q: np.asarray(host_grad(q)[1], dtype=np.float32).reshape(q.shape),
                              jax.ShapeDtypeStruct(p32.shape, jnp.float32), p32, vmap_method="expand_dims")
        return ((jnp.asarray(ct, dtype=jnp.float32)[..., None] * g).astype(p.dtype),)

    log_likelihood.defvjp(fwd, bwd)
    log_likelihood.fitter = twin
    log_likelihood.host = host_loglike
    log_likelihood.host_grad = host_grad
    return log_likelihood
