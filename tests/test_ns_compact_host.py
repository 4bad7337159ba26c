"""CPU: packing of the live rows in mcalf_slice_replace_batch -- what needs no device: the statistics struct against the header's
layout, the refusals of mcalf_set_slice_compact and mcalf_slice_last_stats, the Python surface, and the host driver
`nested.nested_sample`, which the feature leaves alone."""
import ctypes as C
import inspect

import numpy as np
import pytest

import mcalf_amd
import ns_reference as nr
from mcalf_amd import _lib, nested


def test_the_statistics_struct_matches_the_header_layout():
    t = _lib.mcalf_slice_stats_t
    assert C.sizeof(t) == 32
    assert [(name, getattr(t, name).offset) for name, _ in t._fields_] == [
        ("batch", 0), ("rows_launched", 8), ("trials", 16), ("steps", 24), ("compact", 28)]
    assert [getattr(t, name).size for name, _ in t._fields_] == [8, 8, 8, 4, 4]
    assert C.sizeof(_lib.mcalf_slice_opts) == 4 * 4 + 8                       # (the options keep their layout and `reserved`)
    assert _lib.mcalf_slice_opts(1, 2, 3, 0, 5).seed == 5 and _lib.mcalf_slice_opts.reserved.offset == 12


def test_both_entries_refuse_null_and_name_themselves():
    lib = _lib.load()
    st = _lib.mcalf_slice_stats_t()
    for on in (0, 1, 2, -1):
        assert lib.mcalf_set_slice_compact(None, on) == _lib.MCALF_ERR_INVALID
        assert b"mcalf_set_slice_compact: ctx is NULL" in lib.mcalf_last_error(None)
    assert lib.mcalf_slice_last_stats(None, C.byref(st)) == _lib.MCALF_ERR_INVALID
    assert b"mcalf_slice_last_stats: ctx is NULL" in lib.mcalf_last_error(None)
    assert lib.mcalf_slice_last_stats(None, None) == _lib.MCALF_ERR_INVALID
    assert b"mcalf_slice_last_stats" in lib.mcalf_last_error(None)
    assert (st.batch, st.rows_launched, st.trials, st.steps, st.compact) == (0, 0, 0, 0, 0)      # (a refusal writes nothing)


def test_the_python_surface_exists_and_keeps_its_signatures():
    assert {"mcalf_set_slice_compact", "mcalf_slice_last_stats"} <= set(_lib.SYMBOLS)
    fit = mcalf_amd.als_fitter
    assert list(inspect.signature(fit.set_slice_compact).parameters) == ["self", "on"]
    assert list(inspect.signature(fit.slice_stats).parameters) == ["self"]
    sig = inspect.signature(fit.slice_replace_batch)                          # (the setting lives on the context)
    assert list(sig.parameters) == ["self", "U0", "Lmin", "dirs", "nmoves", "max_steps", "seed", "stream_ids"]
    assert hasattr(nested.NestedResult, "rows_launched") and nested.NestedResult.rows_launched is None
    assert nested.NestedResult(rows_launched=7).rows_launched == 7
    sig = inspect.signature(nested.nested_sample)
    assert list(sig.parameters)[:9] == ["loglike_cube", "replace", "ndim", "nlive", "batch", "nmoves", "dlogz", "max_rounds", "seed"]


def test_the_host_driver_returns_what_it_did():
    """`nested.nested_sample` around the numpy restatement of the replacement step, on a 4-D Gaussian: the run of seed 5 with
    60 live points, 15 chains per round and 4 moves, as the driver returned it before `rows_launched` existed.  The counters
    are exact; ln Z is compared to 1e-9, far below anything a change of the driver could hide in."""
    def gauss(U):
        return -0.5 * (((np.asarray(U) - 0.5) / 0.02) ** 2).sum(axis=1)
    res = nested.nested_sample(lambda U: (U.copy(), gauss(U)), nr.replace_with(gauss), 4, 60, batch=15, nmoves=4, dlogz=0.1, seed=5)
    assert (res.rounds, res.nevals, res.unfinished, res.logL.size) == (51, 12292, 0, 825)
    assert res.logZ == pytest.approx(-11.995992261564366, abs=1e-9)
    assert float(res.logL[-1]) == pytest.approx(-0.05890170142262248, abs=1e-12)
    assert res.rows_launched is None                                          # (the numpy `replace` does not say)
