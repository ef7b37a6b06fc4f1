"""CPU: the call-order catalogue (tests/state_cases.py) is complete and its walks are the ones
tests/test_gpu_call_order.py means to run. No GPU: the catalogue is data and closures.
"""
import os

import state_cases as sc
import tpl_amd  # noqa: F401  (the host library: a build that cannot be imported fails here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_entry_point_is_in_the_catalogue():
    """Every tpl_lanczos*, tpl_op_ftk_*device and tpl_op_set_* function of include/tpl.h, and
    tpl_op_enable_timing, is named by a call or a setting, or by NOT_COVERED with a reason: a
    new entry point fails here until the catalogue has it."""
    with open(os.path.join(ROOT, "include", "tpl.h")) as f:
        declared = sc.header_entry_points(f.read())
    assert len(declared) >= 30 and "tpl_lanczos_two_pass_batch_shifted_inv_tol" in declared
    assert "tpl_op_enable_timing" in declared and "tpl_op_set_device_ftk" in declared
    named = {e for c in sc.calls().values() for e in c.entry}
    named |= {v[0] for v in sc.SETTINGS.values()}
    missing = [f for f in declared if f not in named and f not in sc.NOT_COVERED]
    assert not missing, missing
    assert set(sc.NOT_COVERED) == {"tpl_op_tune_order"}
    assert all(len(reason) > 10 for reason in sc.NOT_COVERED.values())
    stale = sorted((named | set(sc.NOT_COVERED)) - set(declared) - {"tpl_op_apply"})
    assert not stale, stale


def test_catalogue_hygiene():
    calls = sc.calls()
    assert len(calls) == len(sc.call_names()) >= 37
    for c in calls.values():
        assert c.entry and c.family in sc.INTERLEAVE and sc.INTERLEAVE[c.family] in calls
        assert calls[sc.INTERLEAVE[c.family]].family != c.family
        for size in c.takes:
            assert len(c.ladder(size)) >= 4, (c.name, size)
        assert c.params() == tuple((z, {"k": sc.K_DEFAULT, "m": sc.M_DEFAULT,
                                        "s": sc.S_DEFAULT}[z]) for z in c.takes)
        assert c.defines & ~sc.FLAG_MASK == 0
    # the first capacity of ensure_state / ensure_batch is max(k, 16)
    assert sc.K_SMALL < 16 < sc.K_BIG and set(sc.K_LADDER) == {1, 2, 7, sc.K_SMALL, sc.K_BIG}
    assert sc.M_LADDER == (1, 2, 5, 64) and sc.S_LADDER == (2, 3, 4, 7)
    for name in sc.FAMILY_CALLS + sc.SETTER_CALLS:
        assert name in calls
    assert {calls[n].family for n in sc.FAMILY_CALLS} == \
        {"single", "multi", "batch", "batch_multi", "tol", "standard"}
    for name, (setter, default, others) in sc.SETTINGS.items():
        assert others and default not in others, name
    assert set(sc.LAYOUT_SETTERS) <= set(sc.SETTING_NAMES)
    assert len(sc.sigmas(64)) == len(set(sc.sigmas(64))) == 64 and len(sc.times(64)) == 64
    for steps in (1, 2, 5, 24):
        assert all(1 <= c <= steps for c in sc.cuts(steps, 64, 3)) and sc.cuts(steps, 5)[0] == steps


def _sizes(steps, size):
    return [dict(arg)[size] for kind, _, arg in steps if kind == "call" and size in dict(arg)]


def test_walks_are_deterministic_and_cover_the_catalogue():
    walks = {seed: sc.walk(seed) for seed in sc.WALK_SEEDS}
    assert len(walks) == 16
    calls = sc.calls()
    seen_calls, seen_setters = set(), set()
    for seed, steps in walks.items():
        assert steps == sc.walk(seed), seed
        assert len(steps) == sc.WALK_STEPS == 40
        for kind, name, arg in steps:
            assert kind in ("call", "set")
            if kind == "call":
                seen_calls.add(name)
                assert arg == calls[name].params(**dict(arg))
                for size, v in arg:
                    assert v in calls[name].ladder(size)
            else:
                seen_setters.add(name)
                assert arg == sc.SETTINGS[name][1] or arg in sc.SETTINGS[name][2]
        ks, ms = _sizes(steps, "k"), _sizes(steps, "m")
        # a k past the first capacity (16) after a call within it; an m above every earlier m
        assert any(k > 16 and min(ks[:i], default=99) <= 16 for i, k in enumerate(ks)), seed
        assert any(i and m > max(ms[:i]) for i, m in enumerate(ms)), seed
        assert any(a[0] == "set" and a[1] in sc.LAYOUT_SETTERS and b[0] == "call"
                   and calls[b[1]].family in sc.BATCH_FAMILIES
                   for a, b in zip(steps, steps[1:])), seed
        n_set = sum(kind == "set" for kind, _, _ in steps)
        assert 2 <= n_set <= 20, (seed, n_set)
    assert seen_calls == set(calls), set(calls) - seen_calls
    assert seen_setters == set(sc.SETTING_NAMES), set(sc.SETTING_NAMES) - seen_setters
    assert len({tuple(map(str, w)) for w in walks.values()}) == 16


def test_tolerance_cases_mix_early_stops_and_full_runs():
    """From the host histories (ftk.inv_residuals on Inputs.dec): at the default sizes and at
    every ladder k from 7 on, and for m = 2, 5 and 64, the shifted solves keep (column 0,
    smallest shift) running to kmax while the largest shift stops within a quarter of K_SMALL;
    in the batch solves column 1 has stopped under every shift by step 6 beside column 0
    that runs to kmax, in the first group of every s. The single inverse solve's met tolerance
    stops column 0 strictly inside the pass, and 0.0 never does."""
    for mat in sc.MATRICES:
        I = sc.inputs(mat)
        assert 0.0 < I.tol_mix < I.tol_met
        for k in (7, sc.K_SMALL, sc.K_BIG):
            assert I.dec(0, k).steps_taken == k and I.dec(1, k).steps_taken == k
            m_met, conv = I.stop(0, k, 0.0, I.tol_met)
            assert conv and 1 < m_met <= 5, (mat, k, m_met)
            assert I.stop(0, k, 0.0, 0.0) == (k, False)
            for m in (2, sc.M_DEFAULT, 64):
                sg = sc.sigmas(m)
                assert sg[0] == sc.SIGMA_MIN and sg[-1] == sc.SIGMA_MAX
                stops0 = [I.stop(0, k, s, I.tol_mix) for s in sg]
                assert stops0[0] == (k, False), (mat, k, m, stops0[0])
                assert stops0[-1][1] and stops0[-1][0] <= sc.K_SMALL // 4, (mat, k, m, stops0[-1])
                assert len({st for st, _ in stops0}) >= 2
                stops1 = [I.stop(1, k, s, I.tol_mix) for s in sg]
                assert all(cv and st <= 6 for st, cv in stops1), (mat, k, m, stops1)
