"""CPU: the Python surface users and the other modules hold on to, pinned.  tests/golden/python_api.json was recorded once by
`surface()` below, from the commit before the Python layer was reorganised (one call idiom, the sampler mixin, the helper
modules); the test recomputes it on the tree it runs in and asserts equality, so a refactor of the layer cannot drop a method,
change a signature or a default, or turn a property into a method unnoticed."""
import inspect
import json
import os
import types

import numpy as np
import pytest

import mcalf_amd
from mcalf_amd import ensemble, nested, tempering
from mcalf_amd.routines import hires_fitter

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "python_api.json")
PACKAGE = mcalf_amd.__name__

# private names tests, tools, dist.py, broker.py and bench.py reach for: on the class ...
CLASS_PRIVATE = ("_ptr", "_rows", "_ensure_prior", "_open_context", "_scale_cube_pc", "_scale_cube_mn", "_check_scalar", "_jax_twin")
# ... and on an instance, set by __init__ (the first row) or by _open_context (the second, absent when it is patched out)
INIT_PRIVATE = ("_ctx", "_lo", "_hi", "_prior_key", "_gauss_sent", "_twin")
CONTEXT_PRIVATE = ("_lib", "_keep", "_p1", "_o1", "_p1_ptr", "_o1_ptr")


def _public_names(module):
    """Sorted names a module offers: no leading underscore, no imported module, nothing imported from outside the package
    (typing, __future__); plain data (tables, constants) counts."""
    return sorted(name for name, obj in vars(module).items()
                  if not name.startswith("_") and not isinstance(obj, types.ModuleType)
                  and str(getattr(obj, "__module__", PACKAGE)).startswith(PACKAGE))


def surface():
    cls = mcalf_amd.als_fitter
    members = {}
    for name in sorted(n for n in dir(cls) if not n.startswith("_") or n in ("__init__", "__call__")):
        obj = getattr(cls, name)
        members[name] = dict(signature=str(inspect.signature(obj)) if callable(obj) else None,
                             property=isinstance(inspect.getattr_static(cls, name), property))
    return dict(als_fitter=members,
                modules={m.__name__.rsplit(".", 1)[-1]: _public_names(m) for m in (hires_fitter, ensemble, nested, tempering)})


def test_public_surface_is_the_recorded_one():
    want = json.load(open(GOLD))
    got = json.loads(json.dumps(surface()))
    assert sorted(got["als_fitter"]) == sorted(want["als_fitter"])
    for name, rec in want["als_fitter"].items():
        assert got["als_fitter"][name] == rec, name
    assert got["modules"] == want["modules"]


def test_private_names_other_code_uses_still_resolve(monkeypatch):
    cls = mcalf_amd.als_fitter
    for name in CLASS_PRIVATE:
        assert callable(getattr(cls, name)), name
    # called unbound on a plain namespace (tests/test_eqw_host.py): plain functions of the class itself
    for name in ("_rows", "calc_N", "calc_N_batch"):
        assert isinstance(inspect.getattr_static(cls, name), types.FunctionType), name
    source = inspect.getsource(cls._open_context)
    for name in CONTEXT_PRIVATE:
        assert f"self.{name}" in source, name
    monkeypatch.setattr(cls, "_open_context", lambda self, dev: None)
    wl = np.linspace(6180, 6220, 50)
    fit = cls(None, [[6180, 6220]], ["CIV 1548"], [1, 1], spectrum=(wl, wl * 0 + 1, wl * 0 + 0.02))
    for name in INIT_PRIVATE:
        assert name in vars(fit), name
    assert fit._ctx is None and fit._prior_key is None and fit._gauss_sent is False and fit._twin is None
    assert fit._lo.shape == fit._hi.shape == (fit.ndim,)


@pytest.mark.parametrize("name", ["_read_ascii_table", "sigma_clipped_median", "LINE_TABLE", "LINE_OVERRIDES", "apply_line_overrides",
                                  "parse_gpriors", "write_equal_weights", "readconfig", "ModelBand", "als_fitter"])
def test_helpers_stay_reachable_from_hires_fitter(name):
    assert hasattr(hires_fitter, name)
