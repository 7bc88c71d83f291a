"""The refusals the actor features share (agx_set_mailbox_priority, agx_set_stash, agx_set_timers,
agx_set_death_watch, agx_set_supervision, agx_set_children and the CRDT kinds from the other side): every
status code and every message text, written out.  The features exclude one another, a multi-rank engine, CRDT
kinds, a ring pool and a started engine; four of them need max_emit = 1."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine, Kind

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 6

FEATURES = ["priority", "stash", "timers", "watch", "supervision"]
ROWS = [[typed.AgxSupervisor(class_mask=1, strategy=typed.SUP_RESTART, max_restarts=-1, within=1)]]
SITE = [(typed.KIND_COMPILED, 0, None)]


def set_feature(eng, name, cls=1):
    if name == "priority":
        eng.set_mailbox_priority(cls, bytes(range(256)))
    elif name == "stash":
        eng.set_stash(cls, 4)
    elif name == "timers":
        eng.set_timers(1)
    elif name == "watch":
        eng.set_death_watch(1)
    else:
        eng.set_supervision(ROWS)


def plain_engine(registered=64, **cfg):
    eng = GpuEngine(EngineConfig(**dict(dict(n_actors=64, bucket_actors=32, throughput=3, capacity=0, n_words=2, max_emit=1),
                                        **cfg)))
    eng.register_range(0, registered, Kind.COUNTER)
    eng.set_mailbox_class(1, 0)
    return eng


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def status_of(call):
    """(status, message) of the refusal"""
    with pytest.raises(AgxError) as e:
        call()
    name, text = str(e.value).split(": ", 1)
    assert name in ("AGX_EINVAL", "AGX_ESTATE")
    return e.value.status, text


# ------------------------------------------------------------------ 1. one feature set, another refused
PAIRS = {  # (set first, refused second)
    ("stash", "priority"): "priority mailboxes need an engine without a deque-based mailbox class (agx_set_stash)",
    ("timers", "priority"): "priority mailboxes need an engine without timers (agx_set_timers)",
    ("watch", "priority"): "priority mailboxes need an engine without death watch (agx_set_death_watch)",
    ("supervision", "priority"): "priority mailboxes need an engine without supervision (agx_set_supervision)",
    ("priority", "stash"): "deque-based mailboxes need an engine without priority tables (agx_set_mailbox_priority)",
    ("timers", "stash"): "deque-based mailboxes need an engine without timers (agx_set_timers)",
    ("watch", "stash"): "deque-based mailboxes need an engine without death watch (agx_set_death_watch)",
    ("supervision", "stash"): "deque-based mailboxes need an engine without supervision (agx_set_supervision)",
    ("priority", "timers"): "timers need an engine without priority tables (agx_set_mailbox_priority)",
    ("stash", "timers"): "timers need an engine without a deque-based mailbox class (agx_set_stash)",
    ("watch", "timers"): "timers need an engine without death watch (agx_set_death_watch)",
    ("supervision", "timers"): "timers need an engine without supervision (agx_set_supervision)",
    ("priority", "watch"): "death watch needs an engine without priority tables (agx_set_mailbox_priority)",
    ("stash", "watch"): "death watch needs an engine without a deque-based mailbox class (agx_set_stash)",
    ("timers", "watch"): "death watch needs an engine without timers (agx_set_timers)",
    ("supervision", "watch"): "death watch needs an engine without supervision (agx_set_supervision)",
    ("priority", "supervision"): "supervision needs an engine without priority tables (agx_set_mailbox_priority)",
    ("stash", "supervision"): "supervision needs an engine without a deque-based mailbox class (agx_set_stash)",
    ("timers", "supervision"): "supervision needs an engine without timers (agx_set_timers)",
    ("watch", "supervision"): "supervision needs an engine without death watch (agx_set_death_watch)",
}


def test_every_ordered_pair_is_listed():
    assert sorted(PAIRS) == sorted((a, b) for a in FEATURES for b in FEATURES if a != b)


@pytest.mark.parametrize("first,second", sorted(PAIRS))
def test_refuses_another_feature(built, first, second):
    eng = plain_engine()
    set_feature(eng, first)
    got = status_of(lambda: set_feature(eng, second))
    set_feature(eng, first)   # (the refused call changed nothing: the first feature can still be set again)
    eng.close()
    assert got == (EINVAL, PAIRS[first, second])


# ------------------------------------------------------------------ 2. children depend on death watch
def test_children_and_death_watch(built):
    eng = plain_engine(registered=32)
    assert status_of(lambda: eng.set_children([(0, 4, 40, 2)], SITE)) == (
        EINVAL, "children need an engine with death watch (agx_set_death_watch first)")
    eng.set_death_watch(2)
    eng.set_children([(0, 4, 40, 2)], SITE)
    assert status_of(lambda: eng.set_death_watch(3)) == (
        EINVAL, "death watch: the slot count cannot change once children are set (agx_set_children)")
    eng.set_death_watch(2)
    eng.close()


# ------------------------------------------------------------------ 3. CRDT kinds, either order
CRDT_FIRST = {
    "priority": "priority mailboxes need an engine without CRDT kinds (one is registered): a state gossip's snapshot handle "
                "carries no message tag",
    "stash": "deque-based mailboxes need an engine without CRDT kinds (one is registered): a state gossip's snapshot row "
             "does not outlive its superstep in a stash",
    "timers": "timers need an engine without CRDT kinds (one is registered)",
    "watch": "death watch needs an engine without CRDT kinds (one is registered)",
    "supervision": "supervision needs an engine without CRDT kinds (one is registered)",
}
CRDT_SECOND = {
    "priority": "CRDT kinds cannot be registered on an engine with a priority mailbox (agx_set_mailbox_priority): a state "
                "gossip's snapshot handle carries no message tag",
    "stash": "CRDT kinds cannot be registered on an engine with a deque-based mailbox (agx_set_stash): a state gossip's "
             "snapshot row does not outlive its superstep in a stash",
    "timers": "CRDT kinds cannot be registered on an engine with timers (agx_set_timers)",
    "watch": "CRDT kinds cannot be registered on an engine with death watch (agx_set_death_watch)",
    "supervision": "CRDT kinds cannot be registered on an engine with supervision (agx_set_supervision)",
}


def crdt_engine():
    """(a GCounter's state takes more than two words: n_words = 8)"""
    eng = GpuEngine(EngineConfig(n_actors=64, bucket_actors=32, throughput=3, capacity=0, n_words=8, max_emit=1))
    eng.set_mailbox_class(1, 0)
    return eng


@pytest.mark.parametrize("name", FEATURES)
def test_refused_with_a_crdt_kind(built, name):
    eng = crdt_engine()
    eng.register_range(0, 64, Kind.GCOUNTER)
    got = status_of(lambda: set_feature(eng, name))
    eng.close()
    assert got == (EINVAL, CRDT_FIRST[name])


@pytest.mark.parametrize("name", FEATURES)
def test_refuses_a_crdt_kind(built, name):
    eng = crdt_engine()
    set_feature(eng, name)
    got = status_of(lambda: eng.register_range(0, 64, Kind.GCOUNTER))
    eng.close()
    assert got == (EINVAL, CRDT_SECOND[name])


# ------------------------------------------------------------------ 4. more than one rank
RANKS = {
    "priority": "priority mailboxes need a single-rank engine (n_ranks is 2; the limit is 1)",
    "stash": "deque-based mailboxes need a single-rank engine (n_ranks is 2; the limit is 1)",
    "timers": "timers need a single-rank engine (n_ranks is 2; the limit is 1)",
    "watch": "death watch needs a single-rank engine (n_ranks is 2; the limit is 1)",
    "supervision": "supervision needs a single-rank engine (n_ranks is 2; the limit is 1)",
}


@pytest.mark.parametrize("name", FEATURES)
def test_refused_on_two_ranks(built, name):
    eng = GpuEngine(EngineConfig(n_actors=64, n_ranks=2, rank=0))
    got = status_of(lambda: set_feature(eng, name, cls=0))
    eng.close()
    assert got == (EINVAL, RANKS[name])


# ------------------------------------------------------------------ 5. max_emit = 2
MAX_EMIT = {
    "stash": "deque-based mailboxes need max_emit = 1 (it is 2): a stash drain stages at most one tell per message",
    "timers": "timers need max_emit = 1 (it is 2): the drain for more evaluates a case more than once, and a timer action "
              "must take effect once",
    "watch": "death watch needs max_emit = 1 (it is 2): the drain for more evaluates a case more than once, and a watch "
             "action must take effect once",
    "supervision": "supervision needs max_emit = 1 (it is 2): the drain for more evaluates a case more than once, and a "
                   "failure must take effect once",
}


@pytest.mark.parametrize("name", sorted(MAX_EMIT))
def test_refused_with_max_emit_2(built, name):
    eng = plain_engine(max_emit=2)
    got = status_of(lambda: set_feature(eng, name))
    eng.close()
    assert got == (EINVAL, MAX_EMIT[name])


def test_priority_takes_max_emit_2(built):
    eng = plain_engine(max_emit=2)
    set_feature(eng, "priority")
    eng.close()


# ------------------------------------------------------------------ 6. after the first run
STARTED = {
    "priority": "set mailbox priorities before the first agx_run",
    "stash": "set stash capacities before the first agx_run",
    "timers": "set timers before the first agx_run",
    "watch": "set death watch before the first agx_run",
    "supervision": "set supervision before the first agx_run",
}


@pytest.mark.parametrize("name", FEATURES)
def test_refused_after_the_first_run(built, name):
    eng = plain_engine()
    eng.tell(0, 1)
    assert eng.run().delivered == 1
    got = status_of(lambda: set_feature(eng, name))
    eng.close()
    assert got == (ESTATE, STARTED[name])


# ------------------------------------------------------------------ 7. a ring pool (reported before `started`)
RING_POOL = {
    "priority": "this engine keeps queued messages in bounded-mailbox rings of 8 slots, drained in arrival order: set "
                "priority tables before the first run",
    "stash": "this engine keeps queued messages in bounded-mailbox rings of 8 slots, which know no stash: set stash "
             "capacities before the first run",
    "timers": "this engine keeps queued messages in bounded-mailbox rings of 8 slots, which know no timers: set timers "
              "before the first run",
    "watch": "this engine keeps queued messages in bounded-mailbox rings of 8 slots, which know no death watch: set death "
             "watch before the first run",
    "supervision": "this engine keeps queued messages in bounded-mailbox rings of 8 slots, which know no supervision: set "
                   "supervision before the first run",
}


@pytest.mark.parametrize("name", FEATURES)
def test_refused_on_a_ring_pool(built, monkeypatch, name):
    monkeypatch.setenv("AGX_RADIX_BITS", "3")
    monkeypatch.setenv("AGX_NO_FUSED", "1")
    monkeypatch.setenv("AGX_RING_APPLY", "1")
    from tests.prio_cases import echo_population
    eng = engine_for(echo_population(3, 8))   # bounded FIFO actors: the per-actor rings come up at the first run
    eng.tell(np.arange(8, dtype=np.uint32), 1 << 24)
    eng.run()
    got = status_of(lambda: set_feature(eng, name, cls=0))
    eng.close()
    assert got == (EINVAL, RING_POOL[name])
