"""CRDT merges on crafted states and the reference's known answers, through the HIP engine.

The seeded CRDT workloads never fill a snapshot row, never populate all 64 lanes of the wave path and
never pass version 15 (DESIGN.md §8 "crafted CRDT states").  The replicas here (tests/crdt_cases.py)
do: 512 live dots, 8-dot elements, versions around 2^16, 2^31 and 2^32, every VersionVector relation
between a sender and its receiver.  Initial states go in through register_range; expectations come
from the plain model (tests/crdt_model.py) over the predicted senders, from the fixtures of
tests/golden (the reference's own answers) and from the BSP oracle, all bit-exact.

Every ORSet scenario runs in three engine shapes, each of which reaches another merge
implementation -- or_only (orset_merge_wave, sparse rows), mixed (crdt_apply, dense rows) and
delta_gossip (dense rows plus deltaVersions within keys of 8) -- on the fused and the multi-pass
pipeline.
"""
import json
import pathlib

import numpy as np
import pytest

from akka_amd.engine import EngineConfig, GpuEngine, Kind, Op
from tests import crdt_cases as C
from tests import crdt_model as M
from tests.test_crdt_model import _gc, _ikeys, run_script
from tests.test_gpu_parity import COUNT_KEYS, assert_same

pytestmark = pytest.mark.gpu

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
ORSET_KAT = json.loads((GOLD / "orset_kat.json").read_text())
D = M.ORSET_WORDS
COUNTER_SHAPES = ("alone", "mixed", "delta_gossip")


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the receptionist fixture)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def run_gpu(w):
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    w.apply_to(eng)
    st = eng.run()
    words, alive = eng.read_state()
    eng.close()
    return st, words, alive


def run_oracle(w):
    from oracle import BspOracle
    ref = BspOracle(**w.engine_kwargs())
    w.apply_to(ref)
    so = ref.run()
    words, alive = ref.read_state()
    return so, words, alive, ref


def assert_parity(w, name):
    """GPU engine = BSP oracle on every counter, state word and alive flag, and conservation."""
    sg, wg, ag = run_gpu(w)
    so, wo, ao, ref = run_oracle(w)
    assert_same(sg, so, (wg, ag), (wo, ao), name)
    assert sg.staged + sg.emitted == sg.delivered + sg.dead_letters + sg.in_flight, name
    return sg, wg, ref


def assert_orset_rows(words, expected, name):
    """Rows of state words against model states, on the 260 data words."""
    for r, exp in enumerate(expected):
        got = words[r, :D]
        if not np.array_equal(got, M.orset_to_words(exp)):
            raise AssertionError(f"{name}: replica {r}: engine {M.orset_from_words(got)} expected {exp}")


# ------------------------------------------------------------------ a. the reference's answers
@pytest.mark.parametrize("shape", C.SHAPES)
def test_orset_merge_kats_through_the_engine(built, pipeline, shape):
    """Each orset_kat.json merge as a 2-replica engine, both directions: the sender is told one
    GossipTick, the receiver's dots and version vector must be the fixture's."""
    delta = shape == "delta_gossip"
    n_total = 2 + (C.N_BESIDE if shape == "mixed" else 0)
    for c in ORSET_KAT["merges"]:
        names = sorted(set(c["this"]["elements"]) | set(c["that"]["elements"]) | set(c["expected_elements"]))
        idx = {k: 7 * i + 3 for i, k in enumerate(names)}  # (spread over the lanes)
        side = {s: M.ORSet({idx[k]: _ikeys(v) for k, v in c[s]["elements"].items()}, _ikeys(c[s]["vvector"]))
                for s in ("this", "that")}
        expected = M.ORSet({idx[k]: _ikeys(v) for k, v in c["expected_elements"].items()},
                           M.vv_merge(side["this"].vvector, side["that"].vvector))  # pointwise max
        for sender in (0, 1):
            states = [side["this"], side["that"]]
            w = C.orset_shape(shape, C.orset_words(states), ([sender], [C.gossip(0)]), fanout=1,
                              seed=C.seed_for(sender, 1 - sender, n_total, delta))
            st, words, _ = run_gpu(w)
            want = list(states)
            want[1 - sender] = expected
            assert_orset_rows(words, want, f"{c['name']} sender {sender}")
            assert st.unhandled == 0 and st.in_flight == 0


class _EngineOps:
    """The five script operations with add / remove / merge done by the engine, one run per op; a
    replica's value is the 260 data words as the engine last left them."""

    def __init__(self, shape):
        self.shape = shape
        self.delta = shape == "delta_gossip"
        self.runs = 0

    def _run(self, words, tells, **kw):
        self.runs += 1
        st, out, _ = run_gpu(C.orset_shape(self.shape, words, tells, **kw))
        assert st.unhandled == 0 and st.in_flight == 0 and st.dead_letters == 0
        return out[:, :D].copy()

    def new(self):
        return np.zeros(D, np.uint64)

    def copy(self, s):
        return s.copy()

    def add(self, s, node, e):  # a host tell to the replica whose id is the node
        words = np.zeros((node + 1, D), np.uint64)
        words[node] = s
        return self._run(words, ([node], [Op.make(Op.ADD, e)]), fanout=1)[node]

    def remove(self, s, e):
        return self._run(s[None, :], ([0], [Op.make(Op.REMOVE, e)]), fanout=1)[0]

    def merge(self, a, b):  # a.merge(b): b gossips to a
        n_total = 2 + (C.N_BESIDE if self.shape == "mixed" else 0)
        return self._run(np.stack([a, b]), ([1], [C.gossip(0)]), fanout=1,
                         seed=C.seed_for(1, 0, n_total, self.delta))[0]


@pytest.mark.parametrize("script", range(len(ORSET_KAT["scripts"])), ids=lambda i: f"script{i}")
@pytest.mark.parametrize("shape", C.SHAPES)
def test_orset_scripts_through_the_engine(built, pipeline, shape, script):
    """Each orset_kat.json script op by op through the engine (ORSetSpec's unit-test programs and its
    eight "A ORSet must" cases): states chain through the GPU from the first op to the last."""
    c = ORSET_KAT["scripts"][script]
    ops = _EngineOps(shape)
    reps, inv = run_script(c["ops"], new=ops.new, add=ops.add, remove=ops.remove, merge=ops.merge, copy=ops.copy)
    assert ops.runs == sum(op[0] in ("add", "remove", "merge") for op in c["ops"])
    for chk in c["checks"]:
        assert {inv[e] for e in M.orset_from_words(reps[chk[1]]).element_set()} == set(chk[2]), (c["name"], chk)
    model, _ = run_script(c["ops"])  # ... and every replica's dots and version vector are the model's
    for name, s in model.items():
        assert M.orset_from_words(reps[name]) == s, (c["name"], name)


def counter_shape(shape, kind, words, tells, **kw):
    """Counter replicas alone, beside a trailing range of ORSet replicas, or with delta-CRDT on."""
    assert shape in COUNTER_SHAPES
    ranges = [(kind, words)]
    if shape == "mixed":
        ranges.append((Kind.ORSET, C.orset_words(C.population(C.N_BESIDE))))
    return C.workload(ranges, tells, delta=shape == "delta_gossip", name=f"crafted_counters_{shape}", **kw)


@pytest.mark.parametrize("shape", COUNTER_SHAPES)
@pytest.mark.parametrize("kind", [Kind.GCOUNTER, Kind.PNCOUNTER])
def test_counter_merge_kats_through_the_engine(built, pipeline, kind, shape):
    """gcounter_kat.json / pncounter_kat.json merges as 2-replica engines, both directions, against the
    fixture's states and values."""
    g = json.loads((GOLD / ("gcounter_kat.json" if kind == Kind.GCOUNTER else "pncounter_kat.json")).read_text())
    n_total = 2 + (C.N_BESIDE if shape == "mixed" else 0)
    for m in g["merges"]:
        a, b = _gc(m["a_ops"]), _gc(m["b_ops"])
        to_words = (lambda x: M.gcounter_to_words(x[0])) if kind == Kind.GCOUNTER else M.pncounter_to_words
        init = np.stack([to_words(a), to_words(b)])
        for sender in (0, 1):
            w = counter_shape(shape, kind, init, ([sender], [C.gossip(0)]), fanout=1,
                              seed=C.seed_for(sender, 1 - sender, n_total, shape == "delta_gossip"))
            st, words, _ = run_gpu(w)
            W = init.shape[1]
            assert np.array_equal(words[sender, :W], init[sender]), m["name"]
            got = words[1 - sender, :W]
            if kind == Kind.GCOUNTER:
                assert got[:g["slots"]].tolist() == m["merged_state"] and not got[g["slots"]:].any(), m["name"]
                assert M.gcounter_value(M.gcounter_from_words(got)) == m["merged_value"], m["name"]
            else:
                pn = M.pncounter_from_words(got)
                assert M.gcounter_value(pn[0]) == m["merged_increments_value"], m["name"]
                assert M.gcounter_value(pn[1]) == m["merged_decrements_value"], m["name"]
                assert M.pncounter_value(pn) == m["merged_value"], m["name"]
            assert st.unhandled == 0 and st.in_flight == 0


# ------------------------------------------------------------------ b. pure merge at the edges
def _orset_kinds(n, shape):
    return [Kind.ORSET] * n + ([Kind.GCOUNTER] * C.N_BESIDE if shape == "mixed" else [])


@pytest.mark.parametrize("n,ba", [(64, 32), (67, 32), (256, 64)])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_pure_merge_of_crafted_replicas(built, pipeline, shape, n, ba):
    """n crafted replicas, every replica told one GossipTick of fanout 2, throughput above the deepest
    inbox.  Replica r must hold model.merge over its own state and those of its predicted senders (the
    order is free: the join laws of tests/test_crdt_model.py); the run must equal the BSP oracle.
    (n = 67: more than one bucket with a short last one, and in delta mode a last key of 3 replicas.)"""
    states = C.population(n)
    C.assert_census(states)
    delta = shape == "delta_gossip"
    kinds = _orset_kinds(n, shape)
    n_total, seed = len(kinds), 7
    snd = C.senders(n_total, seed, 2, 0, delta)
    pairs = [(s, r) for r in range(n) for s in snd[r] if s < n]
    pc = C.pair_census(states, pairs)
    assert all(pc[k] > 0 for k in ("==", "<", ">", "<>", "vanish", "stay")), pc
    assert any(sum(len(d) for d in states[s].elements.values()) == 512 for s, _ in pairs)  # a full row is merged
    ids = np.arange(n_total, dtype=np.uint32)
    w = C.orset_shape(shape, C.orset_words(states), (ids, np.full(n_total, C.gossip(0), np.uint32)), fanout=2, seed=seed,
                      throughput=50, bucket_actors=ba)
    assert max(len(v) for v in snd.values()) + 1 < 50
    sg, words, _ = assert_parity(w, f"pure merge {shape} n={n}")
    expected = [M.merge_all([states[r]] + [states[s] for s in snd[r] if s < n]) for r in range(n)]
    assert_orset_rows(words, expected, f"pure merge {shape}")
    cross = sum(kinds[s] != kinds[r] for r in range(n_total) for s in snd[r])
    assert sg.unhandled == cross and sg.in_flight == 0 and sg.dead_letters == 0
    if shape == "mixed":  # the counters beside them: slot-wise max over their counter senders
        cw = C.counter_population(Kind.GCOUNTER, C.N_BESIDE)
        for r in range(n, n_total):
            exp = cw[r - n].copy()
            for s in snd[r]:
                if s >= n:
                    exp = np.maximum(exp, cw[s - n])
            assert np.array_equal(words[r, :8], exp), r


# ------------------------------------------------------------------ c. queued and forwarded rows
@pytest.mark.parametrize("capacity", [0, 3])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_queued_rows_of_crafted_replicas(built, pipeline, shape, capacity):
    """throughput 1 and three GossipTicks of fanout 2: full 512-dot rows wait in the mailboxes and are
    copied forward across supersteps; with a bounded mailbox some are tail-dropped."""
    n = 64
    states = C.population(n)
    C.assert_census(states)
    n_total = len(_orset_kinds(n, shape))
    ids = np.arange(n_total, dtype=np.uint32)
    w = C.orset_shape(shape, C.orset_words(states), (ids, np.full(n_total, C.gossip(2), np.uint32)), fanout=2, seed=11,
                      throughput=1, capacity=capacity)
    sg, _, ref = assert_parity(w, f"queued rows {shape} C={capacity}")
    rows, full_rows = ref.orset_backlog_census()
    assert full_rows >= 1, (rows, full_rows)  # a full row waited in a mailbox across a superstep
    assert (sg.dead_letters > 0) == (capacity > 0)


# ------------------------------------------------------------------ d. ops in the same drain as merges
def _ops_tells(states):
    """Per replica, in this order: REMOVE e1, ADD e2 (e2 holding 8 dots where the replica has such an
    element), CLEAR (every fourth replica), ADD 63, GossipTick(1), ADD 0."""
    per, plan = {}, []
    for r, s in enumerate(states):
        e1 = min(s.elements, default=31)
        e2 = next((e for e, d in sorted(s.elements.items()) if len(d) == 8 and e != e1), (r * 7 + 1) % 64)
        t = [Op.make(Op.REMOVE, e1), Op.make(Op.ADD, e2)]
        if r % 4 == 0:
            t.append(Op.make(Op.CLEAR, 0))
        t += [Op.make(Op.ADD, 63), C.gossip(1), Op.make(Op.ADD, 0)]
        per[r] = t
        plan.append((e1, e2, r % 4 == 0))
    return per, plan


@pytest.mark.parametrize("throughput", [2, 50])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_ops_in_the_same_drain_as_merges(built, pipeline, shape, throughput):
    n = 64
    states = C.population(n, variant="ops")
    C.assert_census(states)
    per, plan = _ops_tells(states)
    assert sum(len(states[r].elements.get(e2, ())) == 8 for r, (_, e2, _) in enumerate(plan)) > n // 2
    w = C.orset_shape(shape, C.orset_words(states), C.tells_in_order(per), fanout=2, seed=13, throughput=throughput)
    sg, _, _ = assert_parity(w, f"ops and merges {shape} T={throughput}")
    assert sg.in_flight == 0


@pytest.mark.parametrize("shape", C.SHAPES)
def test_ops_without_gossip_equal_the_model(built, pipeline, shape):
    """The same tells with fanout 0: each replica's final state is the model applied in tell order."""
    n = 64
    states = C.population(n, variant="ops")
    C.assert_census(states)
    per, plan = _ops_tells(states)
    w = C.orset_shape(shape, C.orset_words(states), C.tells_in_order(per), fanout=0, seed=13, throughput=2)
    sg, words, _ = assert_parity(w, f"ops without gossip {shape}")
    expected = []
    for r, (s, (e1, e2, clear)) in enumerate(zip(states, plan)):
        node = r % C.NODES
        s = s.remove(e1).add(node, e2)
        if clear:
            s = s.clear()
        expected.append(s.add(node, 63).add(node, 0))
    assert_orset_rows(words, expected, f"ops without gossip {shape}")
    assert sg.unhandled == 0


# ------------------------------------------------------------------ e. counter halves
@pytest.mark.parametrize("shape", COUNTER_SHAPES)
@pytest.mark.parametrize("kind", [Kind.GCOUNTER, Kind.PNCOUNTER])
def test_counter_halves_pure_merge(built, pipeline, kind, shape):
    """Crafted counters whose slots differ in both u32 halves: one GossipTick of fanout 2 by every
    replica; slot-wise Python max over the predicted senders, and the BSP oracle."""
    n, seed = 64, 17
    cw = C.counter_population(kind, n)
    n_total = n + (C.N_BESIDE if shape == "mixed" else 0)
    snd = C.senders(n_total, seed, 2, 0, shape == "delta_gossip")
    C.assert_counter_census(cw, [(s, r) for r in range(n) for s in snd[r] if s < n])
    ids = np.arange(n_total, dtype=np.uint32)
    w = counter_shape(shape, kind, cw, (ids, np.full(n_total, C.gossip(0), np.uint32)), fanout=2, seed=seed, throughput=50)
    sg, words, _ = assert_parity(w, f"counter halves {kind} {shape}")
    W = cw.shape[1]
    for r in range(n):
        exp = [int(x) for x in cw[r]]
        for s in snd[r]:
            if s < n:
                exp = [max(a, int(b)) for a, b in zip(exp, cw[s])]
        assert [int(x) for x in words[r, :W]] == exp, r
    assert sg.in_flight == 0


@pytest.mark.parametrize("capacity", [0, 3])
@pytest.mark.parametrize("shape", COUNTER_SHAPES)
@pytest.mark.parametrize("kind", [Kind.GCOUNTER, Kind.PNCOUNTER])
def test_counter_halves_queued_rows(built, pipeline, kind, shape, capacity):
    n = 64
    cw = C.counter_population(kind, n)
    n_total = n + (C.N_BESIDE if shape == "mixed" else 0)
    C.assert_counter_census(cw, [(s, r) for r in range(n) for s in range(n) if s != r][:512])
    ids = np.arange(n_total, dtype=np.uint32)
    w = counter_shape(shape, kind, cw, (ids, np.full(n_total, C.gossip(2), np.uint32)), fanout=2, seed=19, throughput=1,
                      capacity=capacity)
    sg, _, _ = assert_parity(w, f"counter halves queued {kind} {shape} C={capacity}")
    assert (sg.dead_letters > 0) == (capacity > 0)


# ------------------------------------------------------------------ f. a version wrap is loud
@pytest.mark.parametrize("shape", C.SHAPES)
def test_orset_version_wrap_is_loud(built, pipeline, shape):
    """A replica whose own version-vector entry is 2^32 - 2 takes one ADD: it holds dot 2^32 - 1, and its
    gossip merges correctly into Before and into Concurrent peers.  A second ADD would wrap the u32
    version to 0 -- the add silently lost, the version vector going backwards; the reference's Long
    versions never wrap -- so the engine reports AGX_ERANGE."""
    from oracle import BspOracle
    p = C.pool(variant="wrap")
    adder = p["node3_last"]
    assert adder.vvector[3] == 2**32 - 2
    before = p["full512"]
    concurrent = next(s for s in p.values() if M.vv_compare(s.vvector, adder.vvector) == "<>" and s.elements)
    assert M.vv_compare(before.vvector, adder.vvector) == "<"
    states = [adder if r == 3 else before if r % 2 == 0 else concurrent for r in range(8)]
    C.assert_census(states)
    delta = shape == "delta_gossip"
    n_total = 8 + (C.N_BESIDE if shape == "mixed" else 0)
    fanout = 4

    def peers(seed):
        return {(C.crdt_key_peer if delta else C.crdt_peer)(seed, 3, 0, j, n_total) for j in range(fanout)}
    seed = next(s for s in range(1, 200) if {r % 2 for r in peers(s) if r < 8} == {0, 1})  # both kinds of peer
    e = 5
    w = C.orset_shape(shape, C.orset_words(states), ([3, 3], [Op.make(Op.ADD, e), C.gossip(0)]), fanout=fanout, seed=seed)
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    w.apply_to(eng)
    sg = eng.run()
    words, alive = eng.read_state()
    ref = BspOracle(**w.engine_kwargs())
    w.apply_to(ref)
    so = ref.run()
    assert_same(sg, so, (words, alive), ref.read_state(), f"version wrap {shape}")
    added = adder.add(3, e)
    assert added.elements[e] == {3: 2**32 - 1} and added.vvector[3] == 2**32 - 1
    expected = [added if r == 3 else s.merge(added) if r in peers(seed) else s for r, s in enumerate(states)]
    assert_orset_rows(words, expected, f"version wrap {shape}")
    eng.tell([3], [Op.make(Op.ADD, e + 1)])
    with pytest.raises(Exception, match="AGX_ERANGE"):
        eng.run()
    eng.close()
    ref.tell([3], [Op.make(Op.ADD, e + 1)])
    with pytest.raises(OverflowError):
        ref.run()
