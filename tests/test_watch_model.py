"""The reference model of death watch (tests/watch_model.py), without a GPU: pinned to the frozen FIFO oracle when
no watch is in use, and checked against the known answers restated from the reference's WatchSpec
(tests/golden/watch_kats.json)."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER
from tests import watch_cases as wc
from tests.test_prio_model import run_oracle as run_fifo_oracle, same
from tests.watch_model import DUE, FREE, NOTIFIED, SlotsExhausted, WatchModel


def model_for(w):
    m = WatchModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def run_oracle(w, max_steps=1 << 30):
    """the frozen oracle knows no death watch: the workload without it"""
    saved, w.watch = w.watch, {}
    try:
        return run_fifo_oracle(w, max_steps)
    finally:
        w.watch = saved


def tells(target, *msgs):
    d = np.asarray([m[0] for m in msgs], np.uint32)
    p = np.asarray([(m[1] << 24) | m[2] for m in msgs], np.uint32)
    target.tell(d, p, np.full(d.size, NO_SENDER, np.uint32))


def conserved(st, info):
    return st["staged"] + st["emitted"] + info["terminated"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


# ------------------------------------------------------------------ pinned to the frozen oracle
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("watch", [False, True])
@pytest.mark.parametrize("mix", ["priority_mix", "compiled"])
def test_model_equals_oracle(mix, watch, T):
    """no death watch, and death watch set but never used: the frozen oracle's results"""
    w = wl.priority_mix(2048, seed=5 + T, throughput=T, tables=False) if mix == "priority_mix" else \
        wl.compiled(4096, seed=3, throughput=T)
    assert w.max_emit == 1  # (death watch needs it)
    w.watch = {"n_slots": 2} if watch else {}
    m = model_for(w)
    st = m.run()
    assert same((st, m.read_state(), m.take_outbound()), run_oracle(w)) is None
    info = m.watch_info()
    assert info.pop("ticks") == (st["supersteps"] if watch else 0) and not any(info.values())


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("T", wc.KAT_T)
@pytest.mark.parametrize("name", wc.KAT_NAMES)
def test_kat(name, T):
    wc.check_kat(name, T, wc.run_kat(name, T, model_for(wc.kat_workload(name, T))))


def test_kats_restate_the_spec():
    assert set(wc.KAT_NAMES) == {
        "graceful_termination", "death_pact", "idempotent_watch", "watch_with", "idempotent_watch_with",
        "definition_after_watch_using_unwatch", "redefinition_using_unwatch", "watch_after_watch_with_fails",
        "watch_with_other_message_fails", "watch_with_after_watch_fails"}
    assert len(wc.KATS["left_out"]) == 2 and all("parent" in x for x in wc.KATS["left_out"])
    for s in wc.KATS["scenarios"]:
        assert s["spec_lines"] and len(s["echo"]) == len(s["script"])


# ------------------------------------------------------------------ the rules the scenarios do not reach
def test_latencies():
    """a death at tick s is in the watchers' inboxes at s + 2; a watch at tick s of an actor that died before s, or
    of an id outside the population, is answered at s + 1"""
    m = model_for(wc.mix_workload(96, 3))
    tells(m, (3, wc.MIX_WATCH, 4), (4, wc.MIX_STOP, 0), (5, wc.MIX_WATCH, 300))
    seen = []
    for _ in range(5):
        m.run(1)
        seen.append(m.take_outbound()[1].tolist())
    assert seen == [[], [5], [3], [], []] and m.watch_info()["ticks"] == 3   # (4 died at tick 1: received at 3)
    tells(m, (7, wc.MIX_WATCH, 4))    # tick 4: a watch of an actor dead since tick 1
    m.run(1)
    assert m.read_watch(7)["state"][0] == DUE
    m.run()
    assert m.take_outbound()[1].tolist() == [7] and m.watch_info()["ticks"] == 5


def test_unwatch_before_receipt_discards():
    """the Terminated is in the mailbox behind the Unwatch: discarded at receipt, by generation; a re-watch in
    between takes the slot with the next generation, and the stale envelope does not answer it"""
    m = model_for(wc.mix_workload(64, 1))
    m.start_watch(3, 1, [200])              # due at once: the envelope arrives at tick 1 ...
    tells(m, (3, wc.MIX_WATCH, 200))        # ... behind this unwatch + watch (throughput 1: drained first)
    m.run(1)
    assert m.read_watch(3)["generation"][0] == 2 and m.read_watch(3)["state"][0] == DUE
    st = m.run()
    info = m.watch_info()
    assert info["discarded"] == 1 and info["terminated"] == 2 and m.take_outbound()[2].tolist() == [wc.MIX_ECHO << 24 | 200]
    assert m.read_watch(3)["state"][0] == FREE and st["unhandled"] == 0 and conserved(st, info)


def test_terminated_in_a_full_bounded_mailbox():
    w = wc.mix_workload(64, 1, capacity=2)
    w.watch = {"n_slots": 1, "starts": [(40, 1, [2], 0, None)]}
    m = model_for(w)
    tells(m, (2, wc.MIX_STOP, 0), (40, 9, 1), (40, 9, 2))
    m.run(1)
    tells(m, (40, 9, 3))
    m.run(1)
    tells(m, (40, 9, 4))
    st = m.run()
    info = m.watch_info()
    assert info["terminated"] == 1 and st["dead_letters"] == 1 and m.read_watch(40)["state"][0] == NOTIFIED
    assert conserved(st, info) and st["in_flight"] == 0
    tells(m, (40, wc.MIX_UNWATCH, 2))   # the slot stays notified until unwatch (or stop)
    m.run()
    assert m.read_watch(40)["state"][0] == FREE


def test_slot_exhaustion():
    m = model_for(wc.mix_workload(64, 5, n_slots=2))
    tells(m, (3, wc.MIX_WATCH, 10), (3, wc.MIX_WATCH, 11), (3, wc.MIX_WATCH, 12))
    with pytest.raises(SlotsExhausted):
        m.run()
    assert m.read_watch(3)["watchee"][:2].tolist() == [10, 11] and m.watch_info()["watches"] == 2


def test_a_stop_frees_the_slots():
    m = model_for(wc.mix_workload(64, 5))
    tells(m, (3, wc.MIX_WATCH, 10), (3, wc.MIX_WITH, 11), (3, wc.MIX_STOP, 0))
    m.run()
    assert m.read_watch(3)["state"].tolist() == [FREE] * 4 and m.watch_info()["watching"] == 0
    tells(m, (10, wc.MIX_STOP, 0))
    st = m.run()
    assert m.watch_info()["terminated"] == 0 and m.watch_info()["ticks"] == 2   # (nobody watches: no empty tick)


def test_ticks_under_a_budget():
    w = wl.death_pact_chain(40, bucket_actors=32)
    m = model_for(w)
    for budget, ticks in ((1, 1), (1, 2), (10, 12), (100, 79), (5, 79)):
        st = m.run(budget)
        assert m.watch_info()["ticks"] == ticks and conserved(st, m.watch_info())
    assert m.read_state()[1].sum() == 0 and m.watch_info()["death_pacts"] == 39


@pytest.mark.parametrize("kill", [(5,), (5, 50), (5, 6), (30, 31, 32, 95, 0)])
def test_watch_ring(kill):
    m = model_for(wl.watch_ring(96, kill, bucket_actors=32))
    st = m.run()
    words, alive = m.read_state()
    assert alive.sum() == 96 - len(kill) and words[:, 1].sum() == len(kill) and conserved(st, m.watch_info())
    for a in np.flatnonzero(alive):   # every survivor watches the next survivor
        nxt = next(x % 96 for x in range(a + 1, a + 97) if alive[x % 96])
        assert words[a, 0] == nxt and (nxt == a or m.read_watch(a)["watchee"][0] == nxt)


@pytest.mark.parametrize("n,T", [(96, 1), (70, 5)])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_mix_guard(seed, n, T):
    """the mix the GPU parity test runs is not vacuous, never runs out of slots, stays within one tile per
    bucket, and conserves messages after every run"""
    m = model_for(wc.mix_workload(n, T))
    watching = 0
    for i, (dst, pay) in enumerate(wc.mix_rounds(n, seed)):
        m.tell(dst, pay, np.full(dst.size, NO_SENDER, np.uint32))
        st = m.run(2 if i % 2 else 1 << 30)
        assert conserved(st, m.watch_info())
        watching = max(watching, m.watch_info()["watching"])
    st = m.run()
    info = m.watch_info()
    assert not m.full and info["terminated"] > 5 and info["watches"] > 20 and conserved(st, info)
    assert (m.read_state()[1] == 0).any() and m.max_bucket_inbox(32) <= 2048
    assert watching > 10 and info["discarded"] > 0   # (slots wait for a death between runs; unwatches race envelopes)
