"""-m gpu: mcs_frustum / mcs_search_local_points on the hostile cases of tests/hostile_frustum.py against tests/frustum_model.py, both memory kinds.

Per case: the case's non-vacuity predicate on the model's output first; then in_view, level, view_cos, the untouched fields, visible_inc and n_to_match
bytes equal to the model; proj_x / proj_y bit-equal on every exact-rig case (no atan in them) and by frustum_pack.compare_fields' rule on the Lafida rig
(atol 1e-9 px, identical finiteness, more than 95 % bit-equal); match, nmatches and assigned equal to the model's AND to the model's search run on the
device's own fields; host kind and device kind byte-identical.  A case whose host-kind call is refused by the argument checks (a NULL entry in the mask
pointer array, a stale level outside the pyramid) asserts the refusal and untouched outputs, and runs in device kind.

Measured on an MI355X: the 110 tests of this file take 1.8 s together; the slowest call is geometry.lafida_positions at 0.2 s (the oracle extracts its frame),
every other case is below 20 ms.  No case showed the device and the model apart once the flag rule and the host-side rounding rule were stated as DESIGN.md
section 7 has them."""
import signal

import numpy as np
import pytest

import frustum_pack as P
import hostile_frustum as H

pytestmark = pytest.mark.gpu
STATE = ("in_view", "proj_x", "proj_y", "level", "view_cos")
RUNS = [(n, True) for n in H.CASES] + [(n, False) for n in H.NOMASK_CASES]


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return dict(G=G, pkg=G.mcs, ctx=G.ctx())


@pytest.fixture(autouse=True)
def _time_limit():
    """every test under its own limit: a hung kernel ends the run instead of holding the machine"""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(120)
    yield
    signal.alarm(0)


def check_against_model(case, got, want, desc_masks, where):
    P.compare_fields(got, want, where)
    if case["exact"]:
        fresh = want["fresh"].astype(bool)
        for k in ("proj_x", "proj_y"):
            assert P.same_doubles(got["state"][k][fresh], want["state"][k][fresh]), (where, k)
    assert np.array_equal(got["match"], want["match"]), (where, int((got["match"] != want["match"]).sum()))
    assert got["nmatches"] == want["nmatches"] and np.array_equal(got["assigned"], want["assigned"]), where
    # ... and the model's search on the DEVICE's own fields: a last-place difference of uv can neither cause nor hide a mismatch
    if got["n_to_match"] == 0:
        nm, m, a2 = 0, np.full(got["match"].shape, -1, np.int32), np.ascontiguousarray(case["scene"][6], np.uint8)
    else:
        nm, m, a2 = H.search_on_fields(case["scene"], got["state"], desc_masks=desc_masks)
    assert nm == got["nmatches"] and np.array_equal(m, got["match"]) and np.array_equal(a2, got["assigned"]), where


def same_bytes(a, b, where):
    for k in STATE:
        assert a["state"][k].tobytes() == b["state"][k].tobytes(), (where, k)
    for k in ("match", "assigned", "visible_inc"):
        assert a[k].tobytes() == b[k].tobytes(), (where, k)
    assert (a["nmatches"], a["n_to_match"]) == (b["nmatches"], b["n_to_match"]), where


def assert_refused(env, call, word, where):
    """the call is refused with `word` in the message, and every output still holds what it held"""
    cap, L = env["pkg"]._capi, env["pkg"].lib()
    assert call.run(env["ctx"]) == cap.MCS_ERR_INVALID and word.encode() in L.mcs_last_error(), (where, L.mcs_last_error())
    got = call.read()
    for k in STATE:
        assert got["state"][k].tobytes() == call.init[k].tobytes(), (where, k)
    assert (got["match"] == -9).all() and (got["visible_inc"] == -9).all() and got["n_to_match"] == -9 and got["nmatches"] == -9, where
    assert got["assigned"].tobytes() == call.init["assigned"].tobytes(), where


def run_case(env, case, device, desc_masks=True):
    call = P.Call(env["pkg"], env["G"], case["scene"], device, desc_masks=desc_masks)
    env["pkg"].check(call.run(env["ctx"]))
    if device:
        env["ctx"].synchronize()
    return call.read()


@pytest.mark.parametrize("name,desc_masks", RUNS, ids=[n + ("" if m else "-nomasks") for n, m in RUNS])
def test_hostile_case_matches_the_model_in_both_memory_kinds(env, name, desc_masks):
    case, want = H.get(name), H.model(name, desc_masks)
    case["check"](H.model(name))                       # the branch the case is meant to reach is reached: asserted on the model before the device is asked
    got_d = run_case(env, case, True, desc_masks)
    check_against_model(case, got_d, want, desc_masks, (name, "device"))
    if case["host"]:
        assert_refused(env, P.Call(env["pkg"], env["G"], case["scene"], False, desc_masks=desc_masks), case["host"], name)
        return
    got_h = run_case(env, case, False, desc_masks)
    check_against_model(case, got_h, want, desc_masks, (name, "host"))
    same_bytes(got_h, got_d, name)


@pytest.mark.parametrize("name", ["bounds.distance_edges", "levels.table_nan_inside", "rounding.u0_live", "geometry.lafida_positions", "flags.every_byte"])
def test_frustum_alone_matches_the_model(env, name):
    """mcs_frustum, the entry point without the search (its scale table is an argument of its own)"""
    case, want = H.get(name), H.model(name)
    got = {}
    for device in (False, True):
        call = P.Call(env["pkg"], env["G"], case["scene"], device, search=False)
        env["pkg"].check(call.run(env["ctx"]))
        if device:
            env["ctx"].synchronize()
        got[device] = call.read()
        P.compare_fields(got[device], want, (name, device))
    for k in STATE:
        assert got[False]["state"][k].tobytes() == got[True]["state"][k].tobytes(), (name, k)


def test_device_calls_back_to_back_share_the_scratch(env):
    """a large case, a one-slot case and a 513-slot case enqueued in device kind without a wait in between (the grow-only scratch is reused in stream
    order), then all three checked"""
    calls = []
    for name in H.BACK_TO_BACK:
        case = H.get(name)
        c = P.Call(env["pkg"], env["G"], case["scene"], True)
        env["pkg"].check(c.run(env["ctx"]))
        calls.append((name, case, c))
    env["ctx"].synchronize()
    sizes = [c.n * c.nr for _, _, c in calls]
    assert sizes[0] >= 600 and sizes[1] == 1 and sizes[2] == 513, sizes
    for name, case, c in calls:
        check_against_model(case, c.read(), H.model(name), True, name)


def test_a_refused_call_leaves_outputs_and_scratch_alone(env):
    """on one context: a device-kind call is enqueued, a host-kind call with a stale level outside the pyramid is refused while the first may still run,
    then a hostile case runs in both kinds.  The refusal wrote nothing, and neither neighbour's result moved"""
    first = H.get("contention.idle_interleaved")
    c1 = P.Call(env["pkg"], env["G"], first["scene"], True)
    env["pkg"].check(c1.run(env["ctx"]))
    bad = H.get("stale.levels_outside_the_pyramid")
    assert_refused(env, P.Call(env["pkg"], env["G"], bad["scene"], False), "level", "refused")
    after = H.get("stale.view_cos_radius")
    got_d = run_case(env, after, True)
    got_h = run_case(env, after, False)
    env["ctx"].synchronize()
    check_against_model(first, c1.read(), H.model("contention.idle_interleaved"), True, "before the refusal")
    check_against_model(after, got_d, H.model("stale.view_cos_radius"), True, "after the refusal, device")
    check_against_model(after, got_h, H.model("stale.view_cos_radius"), True, "after the refusal, host")
    same_bytes(got_h, got_d, "after the refusal")
