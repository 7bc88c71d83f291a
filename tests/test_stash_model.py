"""The reference model of the stash (tests/stash_model.py), without a GPU: pinned to the frozen FIFO
oracle when no stash is in use, checked against the reference specs' known answers
(tests/golden/stash_kats.json), and the guards that the scenarios of the GPU file
(tests/test_gpu_stash.py) really exercise what they are meant to."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from tests import stash_cases as sc
from tests.stash_model import StashModel
from tests.test_prio_model import run_oracle as run_fifo_oracle, same


def run_model(w, max_steps=1 << 30):
    m = StashModel(**w.engine_kwargs())
    w.apply_to(m)
    st = m.run(max_steps)
    return m, st, m.read_state(), m.take_outbound()


def run_oracle(w, max_steps=1 << 30):
    """the frozen oracle knows no stash: the workload without its stash capacities"""
    saved, w.stash = w.stash, {}
    try:
        return run_fifo_oracle(w, max_steps)
    finally:
        w.stash = saved


def forwarder_mix(T, stash):
    w = wl.priority_mix(2048, seed=5 + T, throughput=T, tables=False)
    w.stash = {1: 6, 2: 3} if stash else {}
    return w


def switch_mix(T, stash):
    w = wl.compiled(4096, seed=3, throughput=T)
    assert any(b.name in ("on", "off") for b in w.behaviors.behaviors)   # (the switch is part of wl.compiled)
    w.stash = {0: 5} if stash else {}
    return w


# ------------------------------------------------------------------ pinned to the frozen oracle
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("stash", [False, True])
@pytest.mark.parametrize("mix", [forwarder_mix, switch_mix])
def test_model_equals_oracle(mix, stash, T):
    """no stash class, and a stash class that no behaviour uses: the frozen oracle's results"""
    w = mix(T, stash)
    m, st, state, out = run_model(w)
    assert same((st, state, out), run_oracle(w)) is None
    assert m.stash_info() == dict(stashed=0, unstashed=0, overflows=0, held=0, pending=0)


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("T", sc.KAT_T)
@pytest.mark.parametrize("name", sc.KAT_NAMES)
def test_kat(name, T):
    w = sc.kat_workload(name, T)
    m = StashModel(**w.engine_kwargs())
    w.apply_to(m)
    sc.check_kat(name, sc.run_kat(name, T, m))


def test_kat_stash_size_midway():
    """StashSpec.scala:224-225: GetStashSize answers 3 between the stashes and UnstashAll"""
    k = sc.KATS["support_unstash_all"]
    assert sc.payload("GetStashSize:%d" % k["stash_size_midway"]) in sc.payloads(k["expected"]).tolist()


def test_t5_crosses_the_park():
    """the whole script staged at once, T = 5: UnstashAll is processed with GetProcessed behind it in the window"""
    w = sc.kat_workload("support_unstash_all", 5)
    m = StashModel(**w.engine_kwargs())
    w.apply_to(m)
    sc.run_kat("support_unstash_all", 5, m)
    assert sum(t["park_left"] for t in m.trace) == 1


# ------------------------------------------------------------------ no vacuous GPU scenario
@pytest.mark.parametrize("seed,T", sc.POPULATION)
def test_guard_population(seed, T):
    w = wl.stash_gate(2048, seed=seed, throughput=T)
    m, st, state, out = run_model(w)
    info = m.stash_info()
    assert info["stashed"] > 0 and info["unstashed"] > 0 and info["overflows"] > 0
    assert info["held"] > 0 and info["pending"] == 0 and st["in_flight"] == info["held"]
    assert st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]
    assert out[0].size > 0 and (state[1] == 0).any()                       # echoes and stops occur
    assert sum(t["park_left"] for t in m.trace) > 0                        # a release leaves a non-empty park
    assert any(t["pending_no_mail"] for t in m.trace)                      # released entries, empty inbox segment
    ba = sc.POPULATION_BUCKETS[0]                                          # a bucket with such actors only
    assert any({a // ba for a in t["pending_no_mail"]} - {a // ba for a in t["mail"]} for t in m.trace)
    for ba in sc.POPULATION_BUCKETS:                                       # (the tile bound of a stash bucket)
        assert m.max_bucket_inbox(ba) <= sc.TILE
    m3 = run_model(w, 3)
    assert m3[1]["in_flight"] > m3[0].stash_info()["held"]                 # mail in flight after run(3)


def test_guard_pending_only_bucket():
    """GPU test 2: after the Open, actor 99's bucket has released entries and no mail for three supersteps"""
    w = sc.small_gates()
    m = StashModel(**w.engine_kwargs())
    w.apply_to(m)
    m.tell(*sc.gate_msgs(wl.GATE_DATA, [0, 0, 0, 0]))
    m.tell(*sc.gate_msgs(wl.GATE_OPEN, [0]))
    st = m.run()
    assert [t["pending_no_mail"] for t in m.trace[-3:]] == [[sc.LAST]] * 3 and not any(t["mail"] for t in m.trace[-3:])
    assert m.take_outbound()[2].size == 4 and st["in_flight"] == 0


def test_all_open_uses_no_stash():
    w = wl.stash_gate(2048, seed=1, throughput=3, all_open=True)
    m = run_model(w)[0]
    assert m.stash_info()["stashed"] == 0 and m.stash_info()["overflows"] == 0
