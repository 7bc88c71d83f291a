"""The ask pattern on the GPU (agx_set_ask; ActorContextImpl.scala:203-218, AskPattern.scala:109-162): the HIP engine
through the C ABI against the known answers restated from the reference's ActorContextAskSpec and AskSpec
(tests/golden/ask_kats.json) and, snapshot for snapshot, against the model of DESIGN.md §2.9 (tests/ask_model.py,
itself pinned to the timers' model and the known answers by tests/test_ask_model.py), on the fused and the multi-pass
pipelines.  Populations of 80 actors in buckets of 32 (a partial last bucket), throughput 1 and 4.  A snapshot holds
the counters, both infos, every slot of every actor (agx_read_timers / agx_read_asks), the state words, the alive
flags and the outbox in per-sender order; conservation is asserted in every one."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd.engine import EngineConfig, GpuEngine
from tests import ask_cases as ac
from tests.ask_model import AskModel

pytestmark = pytest.mark.gpu

P = ac.payload


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the timers' fixture; NO_FUSED: populations of one digit)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def model_for(w):
    m = AskModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


# ------------------------------------------------------------------ 1. the known answers
@pytest.mark.parametrize("T", ac.KAT_T)
@pytest.mark.parametrize("name", ac.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(ac.kat_workload(name, T))
    got = ac.run_kat(name, T, eng)
    eng.close()
    print(got)
    ac.check_kat(name, T, got)
    assert got == ac.run_kat(name, T, model_for(ac.kat_workload(name, T)))


# ------------------------------------------------------------------ 2. one case per rule, engine against model
@pytest.mark.parametrize("T", (1, 4))
@pytest.mark.parametrize("name", tuple(ac.RULE_CASES))
def test_rule_case(built, pipeline, name, T):
    """asker and target in one bucket and in two, all 80 actors asking in one tick, a PingPong target, a bucket whose
    only work is a timeout, and every rule of §2.9: each snapshot equal to the model's"""
    got = ac.RULE_CASES[name](engine_for, T)
    want = ac.RULE_CASES[name](model_for, T)
    print(got[-1]["counts"], got[-1]["info"], got[-1]["timer_info"])
    assert len(got) == len(want)
    for i, (g, m) in enumerate(zip(got, want)):
        for k in m:
            assert g[k] == m[k], (name, T, i, k)


# ------------------------------------------------------------------ 3. run(budget) in pieces; the pump
def test_budgeted_runs_and_the_pump(built, pipeline):
    """an outstanding ask is a pending single timer: the engine is not quiescent and pump_idle stays scheduled"""
    got = []
    for make in (engine_for, model_for):
        t = make(ac.ask_workload(7, 4, "ignore"))
        ac.tell(t, "Ask0:5")
        steps = []
        for budget in (1, 2, 2, None):
            s = ac.snapshot(t, t.run() if budget is None else t.run(budget))
            s["again"] = t.pump_idle() if make is engine_for else None
            steps.append(s)
        t.close()
        got.append(steps)
    eng, mod = got
    assert [s["again"] for s in eng] == [True, True, True, False]
    assert [s["timer_info"]["ticks"] for s in eng] == [1, 3, 5, 8] and [s["timer_info"]["pending"] for s in eng] == [1, 1, 1, 0]
    assert ac.echoes(eng[-1]) == [P("TimedOut")] and eng[-1]["info"] == dict(asked=1, answered=0, timed_out=1, late=0)
    for g, m in zip(eng, mod):
        for k in m:
            if k != "again":
                assert g[k] == m[k], k


# ------------------------------------------------------------------ 4. the workload
def test_ask_pool_4096(built, pipeline):
    """ask_pool at 4096 actors for 40 ticks against the model: counters, infos, every state word"""
    w = wl.ask_pool(3072, 1024, timeout=4, silent_every=8, period=8, bucket_actors=256)
    eng, mod = engine_for(w), model_for(w)
    out = []
    for t in (eng, mod):
        st = ac.counts(t.run(40))
        ti, ai = t.timer_info(), t.ask_info()
        assert ac.conserved(st, ti), (st, ti)
        words, alive = t.read_state()
        out.append((st, ti, ai, words, alive & 1))
        t.close()
    (st, ti, ai, words, alive), m = out
    print(st, ti, ai)
    assert (st, ti, ai) == m[:3] and np.array_equal(words, m[3]) and np.array_equal(alive, m[4])
    assert ai["asked"] > 3 * 3072 and ai["late"] == 0 and ai["timed_out"] > 0 and ai["answered"] > ai["timed_out"]


def test_ask_retry(built, pipeline):
    w = wl.ask_retry(448, 64, timeout=3, silent_every=2, bucket_actors=64)
    out = []
    for t in (engine_for(w), model_for(w)):
        st = ac.counts(t.run())
        ti, ai = t.timer_info(), t.ask_info()
        assert ac.conserved(st, ti) and st["in_flight"] == 0
        out.append((st, ti, ai, t.read_state()[0].tolist()))
        t.close()
    gave_up = sum(w0 >> 32 for w0, _ in out[0][3][:448])
    assert out[0] == out[1] and out[0][2]["answered"] == 441 and gave_up == 7  # (the 7 clients of the last, silent server have no next one)
