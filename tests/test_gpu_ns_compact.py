"""GPU: packing of the live rows in mcalf_slice_replace_batch (mcalf_set_slice_compact).  The yardstick is the unpacked host
entry on the same context, which tests/test_gpu_ns.py ties to the numpy restatement tests/ns_reference.py: a packed call must
return all six outputs equal to it BY BYTES -- no tolerance -- and every row that ran out of steps must still hold logL > Lmin.
Shapes cross the wave (64) and workgroup (1024) boundaries of the pack kernel's scan, put holes and bad rows where the packed
list and its pad source are formed, and reuse one context across settings and batch sizes so that a stale stamp, slot or row
list would show.  Every case is at most 2048 rows and 300 pixels.

The accounting identities are derived, not measured: an unpacked call launches batch rows for its start and for every step; a
packed one launches batch for the start, count(it - 1) for step it with count(0) = batch, and sum_it count(it) = sum(nevals), so
batch + sum(nevals) <= rows_launched <= 2 batch + sum(nevals); the loop ends with the first step in which no row proposes, which
is step max(nevals) + 1, or at max_steps."""
import ctypes as C

import numpy as np
import pytest

import many_components as mc
import mcalf_amd
from cases import tiny_problem
from mcalf_amd import _lib, nested
from test_gpu_fit import _civ
from test_gpu_ns import INF, _against_reference, _device_call, _evidence_problem, _logl, _same, _starts

pytestmark = pytest.mark.gpu


def _stats_ok(st, compact, batch, nevals, max_steps):
    ne = int(nevals.sum())
    assert st["compact"] == int(compact) and st["batch"] == batch and st["trials"] == ne, st
    assert 0 <= st["steps"] <= min(max_steps, int(nevals.max()) + 1), st
    if compact:
        assert batch + ne <= st["rows_launched"] <= 2 * batch + ne, (st, ne)
    else:
        assert st["rows_launched"] == batch * (1 + st["steps"]), st


def _both(fit, U0, Lmin, D, sid, nmoves, max_steps, seed):
    """The unpacked and the packed call on one context: equal by bytes, the constraint held, the launches accounted for.
    Returns (outputs, stats of the unpacked call, stats of the packed call); the context is left with the setting off."""
    kw = dict(nmoves=nmoves, max_steps=max_steps, seed=seed, stream_ids=sid)
    fit.set_slice_compact(False)
    off = fit.slice_replace_batch(U0, Lmin, D, **kw)
    s_off = fit.slice_stats()
    fit.set_slice_compact(True)
    try:
        on = fit.slice_replace_batch(U0, Lmin, D, **kw)
        s_on = fit.slice_stats()
    finally:
        fit.set_slice_compact(False)
    assert _same(on, off)
    U, theta, L, status, nevals, moves = on
    lmin = np.broadcast_to(np.asarray(Lmin, dtype=float), L.shape)
    assert (L[status == 0] > lmin[status == 0]).all()
    n = U0.shape[0]
    _stats_ok(s_off, False, n, nevals, max_steps)
    _stats_ok(s_on, True, n, nevals, max_steps)
    assert s_on["steps"] == s_off["steps"]
    return on, s_off, s_on


@pytest.fixture(scope="module")
def tiny():
    """(fit, live points, their logL, directions under the median, the median) of cases.tiny_problem(64), evaluated once."""
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        st = fit.slice_stats()
        assert st == dict(batch=0, rows_launched=0, trials=0, steps=0, compact=0)      # before any slice call
        live = np.random.default_rng(1).random((256, fit.ndim))
        L = _logl(fit)(live)
        lmin = float(np.median(L))
        yield fit, live, L, nested.directions(live[L > lmin]), lmin


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 200, 1024, 1025])
@pytest.mark.parametrize("nmoves", [1, 8])
def test_packed_equals_unpacked_under_the_median_constraint(tiny, batch, nmoves):
    fit, live, L, D, lmin = tiny
    U0 = _starts(live, L, lmin, batch, np.random.default_rng(batch + nmoves))
    sid = np.arange(batch, dtype=np.uint64) + np.uint64(2 ** 32 * nmoves)
    got, s_off, s_on = _both(fit, U0, lmin, D, sid, nmoves, 50 * nmoves, seed=batch)
    assert (got[3] == 1).all() and (got[4] >= nmoves).all()
    print(f"batch {batch} nmoves {nmoves}: {s_on['steps']} steps, rows launched {s_off['rows_launched']} unpacked, {s_on['rows_launched']} packed, "
          f"{s_on['trials']} trials")
    if batch > 1 and nmoves == 8:
        assert s_on["rows_launched"] < s_off["rows_launched"]


def test_packed_against_the_numpy_restatement(tiny):
    fit, live, L, D, lmin = tiny
    U0 = _starts(live, L, lmin, 65, np.random.default_rng(12))
    fit.set_slice_compact(True)
    try:
        got = _against_reference(fit, U0, lmin, D, np.arange(65, dtype=np.uint64) + np.uint64(3), 8, 400, seed=6)
        assert fit.slice_stats()["compact"] == 1 and (got[3] == 1).all()
    finally:
        fit.set_slice_compact(False)


def test_holes_bad_starts_and_a_bad_pad_source(tiny):
    fit, live, L, D, _ = tiny
    rng = np.random.default_rng(9)
    full = nested.directions(live)
    lmin = L[:200] - rng.uniform(0.1, 5.0, 200)                         # one constraint per row
    lmin[::7] = L[:200:7]                                                # not above its own logL: a bad start
    lmin[3::7] = L[3:200:7] + 1.0
    sid = np.arange(200, dtype=np.uint64) + np.uint64(5)
    got, _, _ = _both(fit, live[:200].copy(), lmin, full, sid, 8, 400, seed=3)
    bad = np.zeros(200, dtype=bool)
    bad[::7] = bad[3::7] = True
    assert (got[3][bad] == -1).all() and (got[3][~bad] == 1).all() and not got[4][bad].any()
    U0 = live[:65].copy()                                                # row 0, the source of the pads, is a NaN start
    U0[0, 2] = np.nan
    got, _, s_on = _both(fit, U0, L[:65] - 1.0, full, sid[:65], 8, 400, seed=4)
    assert got[3][0] == -1 and (got[3][1:] == 1).all() and np.isnan(got[0][0, 2])
    got, s_off, s_on = _both(fit, live[:65].copy(), INF, full, sid[:65], 8, 400, seed=4)      # every row a bad start
    assert (got[3] == -1).all() and got[0].tobytes() == live[:65].tobytes() and got[2].tobytes() == L[:65].tobytes()
    assert s_on["steps"] == 1 and s_on["trials"] == 0 and s_on["rows_launched"] == 2 * 65 == s_off["rows_launched"]


def test_out_of_steps_no_steps_and_no_moves(tiny):
    fit, live, L, D, lmin = tiny
    U0 = _starts(live, L, lmin, 64, np.random.default_rng(3))
    sid = np.arange(64, dtype=np.uint64)
    got, _, s_on = _both(fit, U0, lmin, D, sid, 8, 3, seed=1)           # the open trial is decided through the slot map
    assert (got[3] == 0).any() and (got[4][got[3] == 0] == 3).all() and (got[2][got[3] == 0] > lmin).all()
    assert s_on["steps"] == 3 and s_on["trials"] == got[4].sum()
    got, _, s_on = _both(fit, U0, lmin, D, sid, 8, 0, seed=1)
    assert (got[3] == 0).all() and got[0].tobytes() == U0.tobytes() and s_on["steps"] == 0 and s_on["rows_launched"] == 64
    got, _, s_on = _both(fit, U0, lmin, D, sid, 0, 50, seed=1)
    assert (got[3] == 1).all() and got[0].tobytes() == U0.tobytes() and s_on["steps"] == 0 and s_on["rows_launched"] == 64


def test_a_lane_that_owns_several_coordinates_in_the_gather():
    with mcalf_amd.als_fitter(None, **mc.many(129)[0]) as fit:
        assert fit.ndim == 129
        live = np.random.default_rng(129).random((4 * 129, 129))
        L = _logl(fit)(live)
        lmin = float(np.median(L))
        U0 = _starts(live, L, lmin, 65, np.random.default_rng(6))
        U0[7, 128] = 2.0                                                # a bad start, by the last coordinate
        D = nested.directions(live[L > lmin])
        got, _, _ = _both(fit, U0, lmin, D, np.arange(65, dtype=np.uint64) + np.uint64(100), 8, 400, seed=4)
        assert got[3][7] == -1 and (np.delete(got[3], 7) >= 0).all() and (got[3] == 1).any()
        assert (np.abs(got[0] - U0)[:, 64:].max(axis=0) > 0.0).all()    # every late coordinate moved in some row


def test_two_lines_floated_resolution_and_continuum():
    kw, _ = _civ(npix=300, specres=(6.0, 9.0), contval=(0.9, 1.1))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.ndim == 15
        live = np.random.default_rng(2).random((128, 15))
        L = _logl(fit)(live)
        lmin = float(np.median(L))
        U0 = _starts(live, L, lmin, 33, np.random.default_rng(4))
        sid = np.arange(33, dtype=np.uint64) * np.uint64(2 ** 33 + 1)
        got, _, _ = _both(fit, U0, lmin, nested.directions(live[L > lmin]), sid, 30, 1500, seed=2 ** 63 + 9)
        assert (got[3] == 1).all()


def _host_call(fit, U0, lmin, D, sid, nmoves, max_steps, seed, theta):
    """mcalf_slice_replace_batch itself, so that theta can be left out."""
    n = U0.shape[0]
    opts = _lib.mcalf_slice_opts(nmoves, max_steps, D.shape[0], 0, seed)
    U0, D = np.ascontiguousarray(U0), np.ascontiguousarray(D)
    Lm = np.full(n, lmin)
    U, T = np.full(U0.shape, -7.0), np.full(U0.shape, -7.0)
    L = np.full(n, -7.0)
    S, N, M = (np.full(n, -7, dtype=np.int32) for _ in range(3))
    rc = fit._lib.mcalf_slice_replace_batch(fit._ctx, U0.ctypes.data, Lm.ctypes.data, D.ctypes.data, sid.ctypes.data, n, C.addressof(opts),
                                            U.ctypes.data, T.ctypes.data if theta else None, L.ctypes.data, S.ctypes.data, N.ctypes.data,
                                            M.ctypes.data)
    assert rc == 0, fit._lib.mcalf_last_error(fit._ctx)
    return U, T, L, S, N, M


def test_one_context_across_settings_and_batch_sizes(tiny):
    fit, live, L, D, lmin = tiny
    U0 = _starts(live, L, lmin, 1025, np.random.default_rng(21))
    sid = np.arange(1025, dtype=np.uint64) + np.uint64(77)
    kw = dict(nmoves=8, max_steps=400, seed=8)
    runs = []
    for on in (True, False, True):                                      # a stale slot, row list or stamp would show in the third
        fit.set_slice_compact(on)
        assert f" ns_compact={int(on)} " in fit.get_config() + " "
        runs.append(fit.slice_replace_batch(U0[:200], lmin, D, stream_ids=sid[:200], **kw))
        assert fit.slice_stats()["compact"] == int(on)
    assert _same(runs[0], runs[1]) and _same(runs[2], runs[1])
    fit.set_slice_compact(False)
    big = fit.slice_replace_batch(U0, lmin, D, stream_ids=sid, **kw)    # 1025 rows unpacked, then 64 of them packed
    fit.set_slice_compact(True)
    try:
        small = fit.slice_replace_batch(U0[900:964], lmin, D, stream_ids=sid[900:964], **kw)
        assert _same(small, [a[900:964] for a in big])
        assert fit.slice_stats()["batch"] == 64
        with_theta = _host_call(fit, U0[:65], lmin, D, sid[:65], 8, 400, 8, theta=True)
        without = _host_call(fit, U0[:65], lmin, D, sid[:65], 8, 400, 8, theta=False)
        assert _same(with_theta, [a[:65] for a in big])
        assert (without[1] == -7.0).all() and _same([a for k, a in enumerate(without) if k != 1], [a[:65] for k, a in enumerate(big) if k != 1])
        with pytest.raises(RuntimeError, match="mcalf_set_slice_compact: on must be 0 or 1"):
            _lib.check(fit._lib.mcalf_set_slice_compact(fit._ctx, 2), fit._ctx)
        assert fit.slice_stats()["compact"] == 1                        # (the refusal changed nothing)
    finally:
        fit.set_slice_compact(False)


def test_several_device_entries_packed_against_one_unpacked(tiny):
    fit, live, L, D, lmin = tiny
    U0 = _starts(live, L, lmin, 1025, np.random.default_rng(22))
    sid = np.arange(1025, dtype=np.uint64) + np.uint64(9)
    kw = dict(nmoves=8, max_steps=400, seed=5)
    fit.set_slice_compact(False)
    ref = fit.slice_replace_batch(U0, lmin, D, stream_ids=sid, **kw)
    with mcalf_amd.als_fitter(None, device=[0, 0, 0], **tiny_problem(64)) as multi:
        multi.set_slice_compact(True)
        assert " ns_compact=1" in multi.get_config()
        got = multi.slice_replace_batch(U0, lmin, D, stream_ids=sid, **kw)
        assert _same(got, ref) and multi.last_launch().devices_used == 3
        st = multi.slice_stats()                                        # the sum over three entries of 342, 342 and 341 rows
        ne = int(ref[4].sum())
        assert st["compact"] == 1 and st["batch"] == 1025 and st["trials"] == ne
        assert 1025 + ne <= st["rows_launched"] <= 2 * 1025 + ne and 0 < st["steps"] <= int(ref[4].max()) + 1
        got = multi.slice_replace_batch(U0[:65], lmin, D, stream_ids=sid[:65], **kw)      # one entry is given all 65 rows
        assert _same(got, [a[:65] for a in ref])
        _stats_ok(multi.slice_stats(), True, 65, ref[4][:65], 400)


def test_the_device_entry_ignores_the_setting(tiny):
    fit, live, L, D, lmin = tiny
    U0 = _starts(live, L, lmin, 65, np.random.default_rng(23))
    sid = np.arange(65, dtype=np.uint64) + np.uint64(100)
    fit.set_slice_compact(True)
    try:
        host = fit.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=60, seed=4, stream_ids=sid)
        assert fit.slice_stats()["compact"] == 1
        rc, dev = _device_call(fit, U0, lmin, D, sid, 8, 60, seed=4)
        assert rc == 0 and _same(dev, host)
        assert fit.slice_stats() == dict(batch=65, rows_launched=61 * 65, trials=-1, steps=60, compact=0)
        rc, dev = _device_call(fit, U0, lmin, D, sid, 0, 60, seed=4)
        assert rc == 0 and fit.slice_stats() == dict(batch=65, rows_launched=65, trials=-1, steps=0, compact=0)
    finally:
        fit.set_slice_compact(False)


def test_the_environment_gives_the_initial_value(monkeypatch):
    monkeypatch.setenv("MCALF_NS_COMPACT", "1")
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        cfg = fit.get_config()
        assert " ns_compact=1 " in cfg and cfg.endswith("[env: MCALF_NS_COMPACT]")
        fit.set_slice_compact(False)
        assert " ns_compact=0 " in fit.get_config()
    monkeypatch.delenv("MCALF_NS_COMPACT")
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        cfg = fit.get_config()
        assert " ns_compact=0 " in cfg and cfg.endswith("[env: none]")


def test_nested_sampling_is_the_same_run_with_fewer_rows():
    kw = _evidence_problem()
    res = []
    for on in (False, True):
        with mcalf_amd.als_fitter(None, **kw) as fit:
            fit.set_slice_compact(on)
            res.append(fit.nested_sample(nlive=256, batch=64, nmoves=8, max_steps=200, seed=0))
    off, on = res
    assert on.logZ == off.logZ and on.rounds == off.rounds and on.nevals == off.nevals and on.unfinished == off.unfinished == 0
    for name in ("cube", "theta", "logL", "logw"):
        assert getattr(on, name).tobytes() == getattr(off, name).tobytes(), name
    print(f"{off.rounds} rounds, {off.nevals} evaluations: rows launched {off.rows_launched} unpacked, {on.rows_launched} packed")
    assert off.rows_launched >= off.nevals and on.rows_launched >= on.nevals
    assert on.rows_launched < off.rows_launched
