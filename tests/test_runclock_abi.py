"""The run clock (cavmd_runclock_*) on a machine WITHOUT a GPU: the header declares exactly its names, in order, and nothing new
under an older prefix; every library exports them and _capi binds them; null handles are refused before a device is needed; a
C99 caller compiles; the Python methods exist; and the numpy restatement of the rules (tests/runclock_mirror.py) against
hand-worked cases -- every edge of a comparison one ulp either side -- and against the two mirrors it is built on wherever no
rule is set."""
import ctypes

import numpy as np
import pytest

import abi_support as abi
import draw_mirror
import runclock_mirror as mirror
import trajectory_mirror



def _bits(x) -> bytes:
    return np.ascontiguousarray(x).tobytes()


NAMES = ["cavmd_runclock_draw_set_end", "cavmd_runclock_draw_finished", "cavmd_runclock_ledger_set_rule",
         "cavmd_runclock_field_set_rule"]


# ---- the names -----------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_names_in_order():
    assert abi.declared("cavmd_runclock_") == sorted(NAMES)
    text = abi.header_text()
    at = [text.index("%s(" % n) for n in NAMES]
    assert at == sorted(at) and text.index("cavmd_trajectory_device_ptr(") < at[0] and at[-1] < text.index("cavmd_profile_enable(")
    raw = " ".join(open(abi.HEADER).read().replace("*", " ").split())
    for words in ("t_end > 0 and elapsed >= t_end", "no block is consumed", "are NOT written", "`finished` (cavmd_draw_state.reserved[0]) becomes 1",
                  "A NaN elapsed compares false", "The last step is not clamped", "src/cavitymd/analysis.py:1230- 1259",
                  "due = rows == 0 || t - last_time >= time_interval", "max_time > 0 && t > max_time: not due",
                  "analysis.py:692-701", "frozen when a launch is captured", "whose address does not change"):
        assert words in raw, words


def test_libraries_export_them_and_capi_binds_them(capi):
    paths = [capi.LIB_PATH, capi.HOOKS_LIB_PATH] + [capi.split_variant_path(name) for name in capi.SPLIT_VARIANTS]
    for path in paths:
        assert {s for s in abi.exported(path) if s.startswith("cavmd_runclock_")} == set(NAMES), path
    assert [n for n in capi._PROTOTYPES if n.startswith("cavmd_runclock_")] == NAMES          # the header's order
    assert set(NAMES) <= set(capi.EXPORTED_SYMBOLS)
    for lib in (capi.load(), capi.load_hooks_build()):
        for n in NAMES:
            assert getattr(lib, n).restype is ctypes.c_int


def test_the_version_is_still_2(capi):
    assert capi.load().cavmd_version() == 2


def test_null_handles_are_refused_without_a_device(capi):
    INV = capi.CAVMD_ERR_INVALID_VALUE
    for lib in (capi.load(), capi.load_hooks_build()):
        t = (ctypes.c_double * 2)(1.0, 2.0)
        n = ctypes.c_uint64(7)
        assert lib.cavmd_runclock_draw_set_end(None, 0, 2, t) == INV
        assert lib.cavmd_runclock_draw_finished(None, None, ctypes.byref(n)) == INV and n.value == 7
        assert lib.cavmd_runclock_ledger_set_rule(None, 1.0, 0.0) == INV
        assert lib.cavmd_runclock_field_set_rule(None, ctypes.c_void_p(64), 64, 1.0, 0.0) == INV


def test_a_c99_caller_compiles_and_runs(capi, tmp_path):
    stdout = abi.run_c99("runclock_abi_check", capi, tmp_path)
    assert "RUNCLOCK-ABI-OK" in stdout, stdout
    sizes, offsets = abi.c_layouts(stdout)
    assert sizes == {"draw_state": 64} and offsets["draw_state"] == dict(elapsed=16, reserved=40)
    assert capi.DrawState.reserved.offset == 40 and capi.DrawState.elapsed.offset == 16


def test_python_methods_exist_and_refuse_cpu_tensors(capi):
    import torch

    import cavitymd
    from cavitymd.step_draw import _STATE_DTYPE
    for cls, names in ((cavitymd.StepDraw, ("set_end_time", "finished", "n_finished")), (cavitymd.BatchEnergyLedger, ("set_time_rule",)),
                       (cavitymd.BatchFieldRecorder, ("set_time_rule", "lag_times")), (capi.FieldRecorder, ("set_time_rule",)),
                       (capi.Draw, ("set_end", "finished")), (capi.Ledger, ("set_time_rule",))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    assert cavitymd.run_until_finished is cavitymd.run_clock.run_until_finished and "run_until_finished" in cavitymd.__all__
    # state() gains the column without moving a byte of cavmd_draw_state
    base = capi.draw_state_dtype()
    assert _STATE_DTYPE.itemsize == base.itemsize == 64 and _STATE_DTYPE.fields["finished"][1] == base.fields["reserved"][1] == 40
    assert all(_STATE_DTYPE.fields[n][1] == base.fields[n][1] for n in base.names)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.StepDraw(1, integrator=torch.zeros((2, 8), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU memory"):
        cavitymd.BatchEnergyLedger(None, [torch.zeros((3, 4), dtype=torch.float64)])
    from cavitymd.field_recorder import _RECORD_DTYPE
    base = capi.field_record_dtype()
    assert _RECORD_DTYPE.itemsize == base.itemsize == 160 and _RECORD_DTYPE.fields["time"][1] == base.fields["reserved"][1] == 24
    with pytest.raises(ValueError, match="check_every"):
        cavitymd.run_until_finished(lambda: None, None, check_every=0)


def test_run_until_finished_counts_chunks():
    """on a stand-in for the draw object: the return is the first chunk end at or past the last finish, max_replays caps it"""
    import cavitymd

    class Clock:
        n_systems = 3

        def __init__(self, finish_after):
            self.replays, self.asked, self.finish_after = 0, 0, finish_after

        def replay(self):
            self.replays += 1

        def n_finished(self):
            self.asked += 1
            return sum(self.replays >= f for f in self.finish_after)

    c = Clock([5, 17, 9])
    assert cavitymd.run_until_finished(c.replay, c, check_every=8) == 24 == c.replays and c.asked == 4
    c = Clock([5, 16, 9])
    assert cavitymd.run_until_finished(c.replay, c, check_every=8) == 16 and c.asked == 3
    c = Clock([5, 17, 9])
    assert cavitymd.run_until_finished(c.replay, c, check_every=8, max_replays=12) == 12 == c.replays
    c = Clock([0, 0, 0])
    assert cavitymd.run_until_finished(c.replay, c) == 0 == c.replays
    c = Clock([1, 1, 10 ** 9])
    assert cavitymd.run_until_finished(c.replay, c, check_every=256, max_replays=0) == 0


# ---- the mirror against hand-worked cases ----------------------------------------------------------------------------------
def _items(B):
    return dict(gamma=np.full(B, 2e-3), kT=np.full(B, 4e-4), set_T=np.full(B, 5e-4), tau=np.array([100.0, 0.0] * B)[:B],
                dof=np.full(B, 3.0), dt_initial=np.full(B, 1.5), tol_target=np.zeros(B), tol_initial=np.zeros(B),
                tol_time_constant=np.zeros(B), dt_min=np.zeros(B), dt_max=np.zeros(B))


def test_end_time_edges():
    below, above = np.nextafter(3.0, 0.0), np.nextafter(3.0, 4.0)
    #                 elapsed == t_end   one ulp below   one ulp above   no end   NaN clock   -0 is none   t_end infinite? refused on the host
    elapsed = np.array([3.0, below, above, 1e300, np.nan, 3.0])
    t_end = np.array([3.0, 3.0, 3.0, 0.0, 3.0, -0.0])
    assert mirror.at_rest(elapsed, t_end).tolist() == [True, False, True, False, False, False]
    B = 6
    it, st = _items(B), mirror.new_state(B)
    st["elapsed"], st["draws"], st["dt"] = elapsed.copy(), np.full(B, 2, dtype=np.uint64), np.full(B, 1.5)
    fixed, none = np.zeros(B, dtype=bool), np.zeros(B, dtype=np.uint64)
    verlet, bussi, new, info = mirror.draw_step(9, it, st, fixed, none, np.zeros(B), t_end)
    rest = info["rest"]
    assert rest.tolist() == [True, False, True, False, False, False] and new["finished"].tolist() == [1, 0, 1, 0, 0, 0]
    one = float(np.array([1], dtype=np.uint64).view(np.float64)[0])
    # an item at rest: dt 0, gamma kept, coeff 0, variates +0, skip 1; c = exp(-0 / tau) = 1, or 0 where tau is 0
    assert _bits(verlet[0]) == _bits(np.array([0.0, 2e-3, 0.0, 0.0, 0.0, 0.0, one, 0.0]))
    assert _bits(bussi[0]) == _bits(np.array([0.0, 0.0, 1.0, 5e-4, one, 0.0, 0.0, 0.0]))
    assert _bits(bussi[2]) == _bits(np.array([0.0, 0.0, 1.0, 5e-4, one, 0.0, 0.0, 0.0]))
    it1 = _items(B)
    _, b1, _, _ = mirror.draw_step(9, it1, dict(st, elapsed=np.full(B, 9.0)), fixed, none, np.zeros(B), np.full(B, 3.0))
    assert b1[:, 2].tolist() == [1.0, 0.0] * 3                                   # tau == 0: c = 0
    # no block consumed, nothing of the state written but `finished`
    for name in mirror.STATE_FIELDS:
        assert _bits(new[name][rest]) == _bits(st[name][rest]), name
    assert (new["draws"][~rest] == 3).all() and _bits(new["elapsed"][1]) == _bits(below + 1.5)
    # the others are draw_mirror's call, bit for bit
    want_v, want_b, want, _ = draw_mirror.step(9, it, {k: st[k] for k in mirror.STATE_FIELDS}, fixed, none, np.zeros(B))
    assert _bits(verlet[~rest]) == _bits(want_v[~rest]) and _bits(bussi[~rest]) == _bits(want_b[~rest])
    # raising t_end: the next call is the one the item would have made
    v2, b2, new2, _ = mirror.draw_step(9, it, new, fixed, none, np.zeros(B), np.full(B, 100.0))
    assert new2["finished"].tolist() == [0, 0, 0, 1, 0, 0] and new2["draws"][0] == 3     # (item 3's clock is at 1e300)
    assert _bits(v2[0]) == _bits(want_v[0]) and _bits(b2[0]) == _bits(want_b[0])


def test_the_draw_mirror_agrees_where_no_end_time_is_set():
    B, seed = 40, 12345
    rng = np.random.default_rng(3)
    it = _items(B)
    it["dof"] = np.array([0.0, 1.0, 2.0, 3.0, 1293.0] * 8)
    it["dt_initial"] = rng.uniform(1.0, 3.0, B)
    fixed, none = np.zeros(B, dtype=bool), np.zeros(B, dtype=np.uint64)
    a, b = draw_mirror.new_state(B), mirror.new_state(B)
    for t_end in (np.zeros(B), np.full(B, 1e300), np.zeros(B)):
        va, ba, a, _ = draw_mirror.step(seed, it, a, fixed, none, np.zeros(B))
        vb, bb, b, info = mirror.draw_step(seed, it, b, fixed, none, np.zeros(B), t_end)
        assert _bits(va) == _bits(vb) and _bits(ba) == _bits(bb) and not info["rest"].any()
        assert all(_bits(a[k]) == _bits(b[k]) for k in mirror.STATE_FIELDS) and (b["finished"] == 0).all()


def test_ledger_rule_edges():
    dt = 0.75
    item = mirror.LedgerItem()
    # the first call records whatever the clock holds
    head = item.call(4, 1, dt, 0.0, 5.0)
    assert head == dict(call=1, row=0, time=5.0, forced=False, slot=0) and item.last_time == 5.0 and item.counters == (1, 1, 0, 1)
    # t - last_time one ulp below the interval: not due; equal to it: due
    t_equal = 5.0 + dt
    assert t_equal - 5.0 == dt                                                  # (exact in this case: hand-checked)
    t_below = np.nextafter(t_equal, 0.0)
    assert t_below - 5.0 < dt
    assert item.call(4, 1, dt, 0.0, t_below) is None and item.counters == (1, 2, 0, 1) and item.last_time == 5.0
    head = item.call(4, 1, dt, 0.0, t_equal)
    assert head["row"] == 1 and head["call"] == 3 and head["slot"] == 1 and item.last_time == t_equal
    # a NaN clock is never due; last_time stays
    assert item.call(4, 1, dt, 0.0, float("nan")) is None and item.counters == (2, 4, 0, 2) and item.last_time == t_equal
    # max_time: t equal to it writes a row, one ulp above does not (whatever the interval says)
    head = item.call(4, 1, dt, 9.0, 9.0)
    assert head is not None and head["time"] == 9.0 and item.counters == (3, 5, 0, 3)
    assert item.call(4, 1, dt, 9.0, np.nextafter(9.0, 10.0) + 5.0) is None
    assert item.call(4, 1, dt, 9.0, np.nextafter(9.0, 10.0)) is None and item.counters == (3, 7, 0, 3) and item.last_time == 9.0
    # the ring wraps; reset zeroes the new word too
    assert item.call(4, 1, dt, 0.0, 20.0)["slot"] == 3 and item.call(4, 1, dt, 0.0, 30.0)["slot"] == 0
    item.reset()
    assert item.counters == (0, 0, 0, 0) and item.last_time == 0.0
    # a first row at a NaN clock lets no further row be due
    assert item.call(4, 1, dt, 0.0, float("nan")) is not None and item.call(4, 1, dt, 0.0, 100.0) is None
    # past max_time the first row is not written either
    fresh = mirror.LedgerItem()
    assert fresh.call(4, 1, dt, 9.0, 9.5) is None and fresh.counters == (0, 1, 0, 0)


def test_the_trajectory_mirror_agrees_where_no_rule_is_set():
    for period in (1, 3):
        a, b = trajectory_mirror.Item(), mirror.LedgerItem()
        for call in range(1, 12):
            want = a.call(4, period, 0.0, 0.25 * call, False)
            got = b.call(4, period, 0.0, 0.0, 0.25 * call)
            assert got == want and b.counters == (a.rows, a.calls, a.phase, a.slot)
        assert b.last_time == 0.0                                               # without a rule the new word is not written
    # and under the rule the decisions are the trajectory's rule 2
    a, b = trajectory_mirror.Item(), mirror.LedgerItem()
    rng = np.random.default_rng(5)
    t = 0.0
    for _ in range(60):
        t += rng.uniform(0.1, 0.9)
        assert b.call(8, 1, 1.3, 0.0, t) == a.call(8, 1, 1.3, t, False)


def test_field_rule_edges():
    CAP, REFS = 8, 3
    item = mirror.FieldItem()
    args = dict(capacity=CAP, period=1, interval=0, max_refs=REFS, time_interval=0.5, ref_time_interval=2.0)
    # the first row is written whatever the clock holds and takes the first reference; both time words follow
    head = item.call(time=10.0, asked=False, **args)
    assert head == dict(call=1, row=0, slot=0, n_references=0, took_reference=True, time=10.0)
    assert (item.last_time, item.last_reference_time, item.ref_rows) == (10.0, 10.0, [0])
    # rows: one ulp below the interval, then equal to it
    assert item.call(time=np.nextafter(10.5, 0.0), asked=False, **args) is None and item.counters == (1, 2, 0, 1, 1, 0)
    head = item.call(time=10.5, asked=False, **args)
    assert head["row"] == 1 and head["call"] == 3 and head["n_references"] == 1 and not head["took_reference"] and head["time"] == 10.5
    # a NaN clock is never due
    assert item.call(time=float("nan"), asked=False, **args) is None
    # references by time: one ulp below reference_time_interval, then equal to it
    head = item.call(time=np.nextafter(12.0, 0.0), asked=False, **args)
    assert head is not None and not head["took_reference"] and item.last_reference_time == 10.0
    head = item.call(time=12.5, asked=False, **args)
    assert head["took_reference"] and head["n_references"] == 1 and item.last_reference_time == 12.5 and item.ref_rows == [0, 3]
    # a forced reference moves last_reference_time: the next one by time counts from it
    head = item.call(time=13.0, asked=True, **args)
    assert head["took_reference"] and head["n_references"] == 2 and item.last_reference_time == 13.0 and item.refs == 3
    # max_references holds
    head = item.call(time=20.0, asked=True, **args)
    assert not head["took_reference"] and head["n_references"] == 3 and item.last_reference_time == 13.0
    item.reset()
    assert item.counters == (0,) * 6 and item.last_time == item.last_reference_time == 0.0
    # reference_time_interval == 0 keeps the row rule: a reference every 2 recorded rows, whatever the clock says
    rows_rule = dict(args, interval=2, ref_time_interval=0.0)
    took = [item.call(time=100.0 * k, asked=False, **rows_rule)["took_reference"] for k in range(6)]
    assert took == [True, False, True, False, True, False] and item.ref_rows == [0, 2, 4]


def test_the_field_mirror_without_a_rule_counts_calls_and_rows():
    """no rule: every period-th call writes a row, references by recorded rows, the time words stay 0 and `time` is +0"""
    item = mirror.FieldItem()
    heads = [item.call(4, 2, 3, 3, 0.0, 0.0, 7.0 * c, False) for c in range(1, 15)]
    written = [h for h in heads if h is not None]
    assert [h["call"] for h in written] == [2, 4, 6, 8, 10, 12, 14] and [h["slot"] for h in written] == [0, 1, 2, 3, 0, 1, 2]
    assert [h["took_reference"] for h in written] == [True, False, False, True, False, False, True]
    assert all(h["time"] == 0.0 for h in written) and item.last_time == item.last_reference_time == 0.0


def test_the_shared_kernel_bodies_find_their_names_in_both_templates():
    """Each new kernel shares its body with the old one as an included file (as a function the body changed the old kernel's
    code).  The body relies on names that one template declares as locals and the other takes as parameters: the list at the
    top of each .inc, the two templates and this table say the same."""
    import os
    import re
    csrc = os.path.join(abi.ROOT, "cav-hoomd_amd", "csrc")
    for header, inc, flag, names in (("cavmd_draw_kernel.hpp", "cavmd_draw_fill_body.inc", "END", ("t_end_all",)),
                                     ("cavmd_ledger_kernel.hpp", "cavmd_ledger_body.inc", "TIMED",
                                      ("period", "time_interval", "max_time", "last_time")),
                                     ("cavmd_field_recorder_kernel.hpp", "cavmd_field_recorder_body.inc", "TIMED", ("period", "rule"))):
        text, body = open(os.path.join(csrc, header)).read(), open(os.path.join(csrc, inc)).read()
        assert text.count('#include "%s"' % inc) == 2, header
        first, second = text.split('#include "%s"' % inc)[:2]
        first = first[first.rindex("template <int BLOCK>"):]                  # the old kernel: flag and names as locals
        second = second[second.index("template <int BLOCK, bool %s>" % flag):]  # the new one: a template flag and parameters
        assert re.search(r"constexpr bool %s = false;" % flag, first), header
        comment = body[:body.index("\n    ")]                                 # the .inc's heading
        for name in (flag,) + names:
            assert re.search(r"\b%s\b" % name, first) and re.search(r"\b%s\b" % name, second), (header, name)
            assert re.search(r"\b%s\b" % name, comment), (inc, name)
            assert re.search(r"\b%s\b" % name, body[len(comment):]), (inc, name)
        assert "if constexpr (%s)" % flag in body
