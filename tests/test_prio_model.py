"""The reference model of the priority mailboxes (tests/prio_model.py), without a GPU: pinned to the
frozen FIFO oracle when no table is set, checked against the reference's own known answers
(tests/golden/priority_mailbox_kats.json), and the guard that every scenario of the GPU file
(tests/test_gpu_priority_mailboxes.py) really depends on the order step."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from tests import prio_cases as pc
from tests.prio_model import PrioModel, per_sender

COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")


def run_model(w, max_steps=1 << 30, tables=True):
    m = PrioModel(**w.engine_kwargs())
    saved = w.mailbox_priorities
    if not tables:
        w.mailbox_priorities = {}
    try:
        w.apply_to(m)
    finally:
        w.mailbox_priorities = saved
    st = m.run(max_steps)
    return m, st, m.read_state(), m.take_outbound()


def run_oracle(w, max_steps=1 << 30):
    from oracle import BspOracle
    ref = BspOracle(**w.engine_kwargs())
    saved, w.mailbox_priorities = w.mailbox_priorities, {}
    try:
        w.apply_to(ref)
    finally:
        w.mailbox_priorities = saved
    st = ref.run(max_steps)
    out = ref.take_outbound()
    state = ref.read_state()
    ref.close()
    return st, state, out


def same(a, b):
    """(counters, (words, alive), outbox) x 2 -> None or what differs"""
    for k in COUNT_KEYS:
        if a[0][k] != b[0][k]:
            return f"{k}: {a[0][k]} != {b[0][k]}"
    if not np.array_equal(a[1][1], b[1][1]):
        return "alive"
    if not np.array_equal(a[1][0], b[1][0]):
        return f"state at {np.nonzero((a[1][0] != b[1][0]).any(axis=1))[0][:8]}"
    if a[2][0].size != b[2][0].size or not np.array_equal(per_sender(*a[2]), per_sender(*b[2])):
        return "outbox"
    return None


def order_differs(a, b):
    """a state word or an outbox sequence differs"""
    return (not np.array_equal(a[1][0], b[1][0])) or a[2][0].size != b[2][0].size or \
        not np.array_equal(per_sender(*a[2]), per_sender(*b[2]))


# ------------------------------------------------------------------ pinned to the frozen oracle
@pytest.mark.parametrize("T,C", [(1, 0), (3, 0), (5, 4)])
def test_model_equals_oracle_mailbox_mix(T, C):
    w = wl.mailbox_mix(4096, seed=T + C, throughput=T, capacity=C)
    assert same(run_model(w)[1:], run_oracle(w)) is None


def test_model_equals_oracle_compiled():
    w = wl.compiled(6000, seed=3, throughput=3)
    assert same(run_model(w)[1:], run_oracle(w)) is None


def test_model_equals_oracle_priority_mix_fifo():
    w = wl.priority_mix(2048, seed=5, tables=False)
    assert same(run_model(w)[1:], run_oracle(w)) is None


def test_constant_table_is_fifo():
    for T, C in pc.CONSTANT_TC[:2]:
        w = pc.constant_mix(T, C)
        w.tells = tuple(x[:6000] for x in w.tells)  # (a slice: the model is slow)
        assert same(run_model(w)[1:], run_model(w, tables=False)[1:]) is None


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("T", pc.KAT_T)
@pytest.mark.parametrize("capacity", pc.KAT_CAPACITY)
def test_stable_priority_kat(T, capacity):
    w, exp, dead = pc.stable_kat(T, capacity)
    _, st, _, (d, s, p) = run_model(w)
    assert np.array_equal(p, exp)
    assert (s == pc.ECHO_ACTOR).all() and (d == pc.N_KAT).all()
    assert st["dead_letters"] == dead and st["delivered"] == exp.size and st["in_flight"] == 0


def test_stable_priority_kat_is_the_specs_order():
    """unbounded: lo ++ hi ++ Result (StablePriorityDispatcherSpec.scala:91-93)"""
    sent = pc.KATS["stable_priority"]["send_order"]
    assert sorted(sent) == list(range(1, 201))
    _, exp, dead = pc.stable_kat(5, 0)
    assert dead == 0
    assert (exp >> 24).tolist() == list(range(1, 101)) + [x for x in sent if x > 100] + [pc.RESULT_TAG]


@pytest.mark.parametrize("T", pc.KAT_T)
def test_priority_kat(T):
    """PriorityDispatcherSpec.scala:58-86: priority = the integer, 1..100 shuffled -> ascending, then Result"""
    k = pc.KATS["priority"]
    sent = [int(x) for x in k["send_order"]] + [pc.RESULT_TAG]
    w = pc.echo_population(T, 0)
    w.tells = (np.full(len(sent), pc.ECHO_ACTOR, np.uint32), np.full(len(sent), 0xFFFFFFFF, np.uint32),
               np.asarray(sent, np.uint32) << np.uint32(24))
    w.mailbox_priorities = {0: bytes(range(256))}
    p = run_model(w)[3][2]
    assert (p >> 24).tolist() == list(range(1, 101)) + [pc.RESULT_TAG]


@pytest.mark.parametrize("T", pc.KAT_T)
@pytest.mark.parametrize("capacity", [0, 1000])
def test_control_aware_kat(T, capacity):
    w, exp = pc.control_kat(capacity)
    w.throughput = T
    assert np.array_equal(run_model(w)[3][2], exp)


def test_overtake_a_backlog():
    st, p, normal, control = pc.overtake(PrioModel(**pc.echo_population(2, 0).engine_kwargs()))
    # superstep 1 drains normal[0:2]; superstep 2 starts with the two control messages
    assert p.tolist() == normal[:2].tolist() + control.tolist() + normal[2:].tolist()
    assert st["delivered"] == 8 and st["supersteps"] == 4


# ------------------------------------------------------------------ no vacuous GPU scenario
@pytest.mark.parametrize("T", pc.KAT_T)
@pytest.mark.parametrize("capacity", pc.KAT_CAPACITY)
def test_guard_stable_kat(T, capacity):
    w, _, _ = pc.stable_kat(T, capacity)
    assert order_differs(run_model(w)[1:], run_model(w, tables=False)[1:])


@pytest.mark.parametrize("capacity", [0, 1000])
def test_guard_control_kat(capacity):
    w, _ = pc.control_kat(capacity)
    assert order_differs(run_model(w)[1:], run_model(w, tables=False)[1:])


@pytest.mark.parametrize("seed,T", pc.POPULATION)
def test_guard_population(seed, T):
    w = wl.priority_mix(2048, seed=seed, throughput=T)
    m, st, state, out = run_model(w)
    assert order_differs((st, state, out), run_model(w, tables=False)[1:])
    assert st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]
    assert out[0].size > 0 and st["dead_letters"] > 0 and (state[1] == 0).any()  # echoes, drops and stops all occur
    sizes = np.stack(m.inbox_sizes)
    assert ((sizes >= 2) & (sizes <= 40)).sum() > 100  # many actors hold 2-40 messages
    for ba in pc.POPULATION_BUCKETS:  # (the tile bound of a prioritised bucket)
        assert m.max_bucket_inbox(ba) <= pc.TILE


@pytest.mark.parametrize("T,C", pc.CONSTANT_TC)
def test_constant_mix_fits_the_tile(T, C):
    """the buckets of test 5 of the GPU file stay within one tile (all of them hold prioritised actors)"""
    w = pc.constant_mix(T, C)
    m = run_model(w, tables=False)[0]
    assert m.max_bucket_inbox(pc.CONSTANT_BUCKET_ACTORS) <= pc.TILE


def test_guard_presorted():
    w, ref = pc.presorted()
    a = run_model(w, 1)[1:]
    assert order_differs(a, run_model(w, 1, tables=False)[1:])
    assert same(a, run_oracle(ref, 1)) is None  # the model itself passes the GPU file's test 6
