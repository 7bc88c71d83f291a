"""The reference model of supervision (tests/supervision_model.py), without a GPU: pinned to the frozen FIFO oracle
on compiled workloads with no failing case, and checked against the known answers restated from the reference's
SupervisionSpec (tests/golden/supervision_kats.json)."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from tests import supervision_cases as sc
from tests.supervision_model import NO_DEADLINE, SupervisionModel
from tests.test_prio_model import run_oracle as run_fifo_oracle, same


def model_for(w):
    m = SupervisionModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def run_oracle(w, max_steps=1 << 30):
    """the frozen oracle knows no supervision: the workload without it"""
    saved, w.supervision = w.supervision, {}
    try:
        return run_fifo_oracle(w, max_steps)
    finally:
        w.supervision = saved


def conserved(st):
    return st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


# ------------------------------------------------------------------ pinned to the frozen oracle
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("supervised", [False, True])
@pytest.mark.parametrize("mix", ["priority_mix", "compiled"])
def test_model_equals_oracle(mix, supervised, T):
    """no supervision, and supervision set with no failing case: the frozen oracle's results"""
    w = wl.priority_mix(2048, seed=5 + T, throughput=T, tables=False) if mix == "priority_mix" else \
        wl.compiled(4096, seed=3, throughput=T)
    assert w.max_emit == 1  # (supervision needs it)
    restart = typed.AgxSupervisor(class_mask=0xFFFFFFFF, strategy=typed.SUP_RESTART, max_restarts=-1, within=1)
    w.supervision = {"rows": [[restart]] * max(w.behaviors.n_behaviors if w.behaviors else 1, 1)} if supervised else {}
    m = model_for(w)
    st = m.run()
    assert same((st, m.read_state(), m.take_outbound()), run_oracle(w)) is None
    info = m.supervision_info()
    assert info.pop("ticks") == st["supersteps"]
    assert info == dict(failures=0, resumes=0, restarts=0, stops=int((m.read_state()[1] == 0).sum()) if supervised else 0)


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("T", sc.KAT_T)
@pytest.mark.parametrize("name", sc.KAT_NAMES)
def test_kat(name, T):
    sc.check_kat(name, T, sc.run_kat(name, T, model_for(sc.kat_workload(name, T))))


def test_kats_restate_the_spec():
    assert set(sc.KAT_NAMES) == {
        "receive_message", "stop_when_no_supervise", "stop_when_unhandled_exception", "restart_when_handled_exception",
        "resume_when_handled_exception", "nesting_for_different_exceptions", "stop_after_restart_retries_limit",
        "reset_retry_limit_after_within", "stop_at_first_exception_when_limit_is_0"}
    for s in sc.KATS["scenarios"]:
        assert s["spec"] and len(s["echo"]) == len(s["script"])


# ------------------------------------------------------------------ the rules the scenarios do not reach
def test_limit_passes_to_the_outer_entry_and_an_outer_restart_clears_the_inner_counts():
    sup = (("E1", [1, 50]), ("E1", "resume"), ("E3", "restart"))
    m = model_for(sc.mix_workload(64, 1, sup))
    E1, E3 = 0, 2
    sc.tells(m, (3, sc.MIX_INC, 1), (3, sc.MIX_THROW, E1))
    m.run()   # ticks 1, 2: the inner entry restarts
    r = m.read_supervision(3)
    assert r["count"].tolist() == [1, 0, 0, 0] and r["remaining"].tolist() == [50, NO_DEADLINE, NO_DEADLINE, NO_DEADLINE]
    sc.tells(m, (3, sc.MIX_INC, 1), (3, sc.MIX_THROW, E1), (3, sc.MIX_ECHO, 0))
    m.run()   # the limit of 1 is reached and time is left: rethrown to the resume, the state stays
    assert m.supervision_info()["resumes"] == 1 and m.take_outbound()[2].tolist() == [sc.MIX_PRE << 24 | 1, sc.MIX_ECHO << 24 | 1]
    sc.tells(m, (3, sc.MIX_THROW, E3))
    m.run()   # the outer restart re-creates the inner interceptors
    r = m.read_supervision(3)
    assert r["count"].tolist() == [0, 0, 1, 0] and r["remaining"][0] == NO_DEADLINE
    sc.tells(m, (3, sc.MIX_THROW, E1))
    st = m.run()
    info = m.supervision_info()
    assert m.read_supervision(3)["count"].tolist() == [1, 0, 1, 0] and info["restarts"] == 3 and info["stops"] == 0
    assert info["ticks"] == st["supersteps"] == 7 and conserved(st)


def test_time_does_not_pass_between_runs():
    """a window that spans two runs: run(1) steps and one run() give the same result"""
    out = []
    for budgets in ((1, 1, 1, 1, 1, 1), (1 << 30,)):
        m = model_for(sc.mix_workload(64, 1))
        sc.tells(m, *[(3, sc.MIX_THROW, 0)] * 2, (3, sc.MIX_INC, 0), (3, sc.MIX_INC, 0), *[(3, sc.MIX_THROW, 0)] * 2)
        for b in budgets:
            st = m.run(b)
        out.append((sc.counts(st), sc.snapshot(m, range(64))))
    assert out[0] == out[1] and out[0][1]["info"]["restarts"] == 4 and out[0][1]["alive"][3] == 1


def test_a_failure_that_stops_a_bounded_mailbox():
    m = model_for(sc.mix_workload(64, 2, capacity=4))
    sc.tells(m, (3, sc.MIX_INC, 1), (3, sc.MIX_THROW, 2), *[(3, sc.MIX_INC, 2)] * 4)   # E3 is not caught
    st = m.run()
    # 6 tells, 4 admitted; tick 1 drains 2 (the failure stops the actor), the 2 queued ones die at tick 2
    assert st["delivered"] == 2 and st["dead_letters"] == 4 and conserved(st) and m.read_state()[1][3] == 0
    assert m.take_outbound()[2].tolist() == [sc.MIX_POST << 24 | 1]


@pytest.mark.parametrize("n", [96, 70])
def test_shapes_guard(n):
    """the script the GPU parity test runs is not vacuous and conserves messages after every run"""
    m = model_for(sc.mix_workload(n, 3))
    for i, st in enumerate(sc.shapes_script(n)(m)):
        assert conserved(st)
        if i == 0:   # actor 7 became `second` and failed there: back in `first`, the count re-created
            assert m.kind[7] == m.init_kind[7] and m.read_state()[0][7, 0] == 0
        if i == 2:   # ... where an Inc counts 1, not 10
            assert m.kind[7] == m.init_kind[7] and m.read_state()[0][7, 0] == 1
    info = m.supervision_info()
    assert info["restarts"] >= 10 and info["stops"] >= 4 and m.read_state()[1][[0, 6, 7, 8]].sum() == 0
    assert m.max_bucket_inbox(32) <= 2048


def test_flaky_workers():
    w = wl.flaky_workers(4096, bucket_actors=32)
    m = model_for(w)
    st = m.run()
    info = m.supervision_info()
    d, s, p = m.take_outbound()
    # (a poison job behind the one that stopped its worker is a dead letter, not a failure)
    assert conserved(st) and st["in_flight"] == 0 and 0 < info["failures"] <= w.n_tells - 4096
    assert info["restarts"] + info["stops"] == info["failures"] and info["stops"] > 0
    assert (p >> 24 == wl.FW_RESTARTED).sum() == info["restarts"] and (p >> 24 == wl.FW_STOPPED).sum() == info["stops"]
    assert (d == 4096 + s % 4).all()   # every worker reports to its own monitor: word 1 survives the restarts
