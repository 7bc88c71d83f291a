"""Delta replication of LWWMap replicas (agx_set_lwwmap_delta: ORMap.DeltaOp groups, causal delivery, full-state
gossip as the repair path) through the HIP engine, against the plain model of tests/lwwmap_delta_model.py: bit-exact
on every state word (data, deltaVersions, selector words, the ring), alive flag and Stats counter, after every leg
of a run.  The seeded cases and what each exercises are in tests/lwwmap_delta_cases.py; each claim is asserted on the
model run before the engine is compared."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.ddata import LWWMap as DecodedMap
from akka_amd.engine import EngineConfig, GpuEngine, Kind, Op
from tests import lwwmap_delta_cases as CS
from tests import lwwmap_delta_model as D
from tests.test_gpu_parity import COUNT_KEYS

pytestmark = pytest.mark.gpu

W = D.DELTA_WORDS
AGX_ECAPACITY = 5


def assert_same(eng, sg, model, so, name):
    for k in COUNT_KEYS:
        assert getattr(sg, k) == so[k], f"{name}: {k} gpu={getattr(sg, k)} model={so[k]}"
    assert sg.staged + sg.emitted == sg.delivered + sg.dead_letters + sg.in_flight, name
    words, alive = eng.read_state()
    mw, ma = model.read_state()
    assert np.array_equal(alive, ma), f"{name}: alive differs"
    diff = np.nonzero((words[:, :W] != mw[:, :W]).any(axis=1))[0]
    if diff.size:
        r = int(diff[0])
        cols = np.nonzero(words[r, :W] != mw[r, :W])[0]
        raise AssertionError(f"{name}: {diff.size} replicas differ, first {r} at words {cols[:8]}: "
                             f"engine {words[r, cols[:8]]} model {mw[r, cols[:8]]}")
    return words


def run_case(name, legs=(4, None), **cfg):
    """The case through the model (its claims asserted first) and the engine, leg by leg: run(4), then to
    quiescence; after every leg all counters and all state words must agree.  Returns (words, model)."""
    factory, extra, _ = CS.CASES[name]
    w = factory()
    model = D.LwwDeltaModel(**w.engine_kwargs())
    w.apply_to(model)
    mstats = [model.run(*([leg] if leg is not None else [])) for leg in legs]
    # (the model again, leg by leg beside the engine: the first pass was the census)
    CS.assert_claims(name, model)
    model = D.LwwDeltaModel(**w.engine_kwargs())
    w.apply_to(model)
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **extra, **cfg)))
    try:
        w.apply_to(eng)
        words = None
        for i, leg in enumerate(legs):
            args = [leg] if leg is not None else []
            sg, so = eng.run(*args), model.run(*args)
            assert so == mstats[i]
            words = assert_same(eng, sg, model, so, f"{name} leg {i}")
        assert sg.in_flight == 0
    finally:
        eng.close()
    return words, model


@pytest.mark.parametrize("n", [8, 9, 20, 72])
def test_populations(built, n):
    """One key; a one-member last key (replica 8 alone: no peers, ticks still run); a four-member last key; more
    replicas than one block's waves."""
    words, model = run_case(f"pop_{n}")
    if n == 9:
        assert model.ctr[8] > 0 and not any(model.sent[8]) and not any(model.dv[8])


def test_population_of_4096(built):
    run_case("pop_4096")


@pytest.mark.parametrize("T,C", [(5, 0), (1, 0), (2, 6)])
def test_throughput_and_capacity(built, T, C):
    """Capped drains make DeltaPropagations queue (their rows are copied forward by their used length); the bounded
    mailbox drops some, which leaves causal gaps that full-state gossip repairs."""
    run_case(f"caps_T{T}_C{C}")


@pytest.mark.parametrize("T,C", [(1, 0), (2, 6)])
@pytest.mark.parametrize("poison", ["0", "255"])
def test_capped_cases_with_a_poisoned_heap(built, monkeypatch, T, C, poison):
    """The capped cases again with every fresh row allocation filled with a byte: a row word read and never written
    shows as a difference from the model."""
    monkeypatch.setenv("AGX_HEAP_POISON", poison)
    run_case(f"caps_T{T}_C{C}")


@pytest.mark.parametrize("max_delta", [1, 2, 50])
def test_max_delta_size(built, max_delta):
    run_case(f"max_delta_{max_delta}")


def test_max_delta_size_1_with_writers(built):
    """Writer ticks under max-delta-size 1: groups of one seqNr are told, longer ones are placeholders."""
    run_case("max_delta_1_writers")


@pytest.mark.parametrize("ba", [32, 512, 2048])
def test_bucket_widths(built, ba):
    run_case(f"bucket_{ba}")


def test_skew_path(built):
    """One 2048-actor bucket with about 7 messages per replica a superstep: over one LDS tile, the skew launch."""
    run_case("skew", msg_capacity=1 << 16)


def test_multipass(built, monkeypatch):
    monkeypatch.setenv("AGX_RADIX_BITS", "3")
    run_case("multipass")


def test_multipass_without_the_fused_pipeline(built, monkeypatch):
    monkeypatch.setenv("AGX_RADIX_BITS", "3")
    monkeypatch.setenv("AGX_NO_FUSED", "1")
    run_case("multipass")


@pytest.mark.parametrize("name", ["reverse_clock", "base_2_41"])
def test_clocks_and_wide_timestamps(built, name):
    run_case(name)


def test_ring_of_64_unsent_seqnrs(built):
    words, model = run_case("ring_64", legs=(None,))
    assert all(DecodedMap.from_words(words[a]).delta_versions[0] == 64 for a in range(1, 8))


def test_ring_of_65_unsent_seqnrs_is_loud(built):
    w = CS.ring_fill(65)
    model = D.LwwDeltaModel(**w.engine_kwargs())
    w.apply_to(model)
    model.run()
    assert model.capacity_error
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    try:
        w.apply_to(eng)
        with pytest.raises(AgxError) as ei:
            eng.run()
        assert ei.value.status == AGX_ECAPACITY
    finally:
        eng.close()


@pytest.mark.parametrize("case", CS.KATS["engine_scripts"], ids=lambda c: c["name"])
def test_kat_scripts_through_the_engine(built, case):
    """Each script op by op, one engine run per step; after every step every replica's 880 words are the model's."""
    eng = GpuEngine(EngineConfig(n_actors=case["replicas"], n_words=W, max_emit=4, bucket_actors=32))
    try:
        got = CS.run_engine_script(case, eng)
    finally:
        eng.close()
    want = CS.run_engine_script(case, D.LwwDeltaModel(case["replicas"], max_emit=4))
    assert len(got) == len(want)
    for i, (g, m) in enumerate(zip(got, want)):
        assert np.array_equal(g, m), f"{case['name']}: after run {i}: replicas {np.nonzero((g != m).any(axis=1))[0]} differ"


def test_set_lwwmap_in_either_order(built):
    """agx_set_lwwmap before or after agx_set_lwwmap_delta: the same run."""
    w = wl.crdt_lwwmap_delta(24, rounds=4, ops_per_replica=2, gossip_rounds=2, clock="reverse", base=77, bucket_actors=32)
    out = []
    for delta_first in (False, True):
        eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
        try:
            eng.register_range(0, 24, Kind.LWWMAP)
            eng.set_gossip(*w.gossip)
            if delta_first:
                eng.set_lwwmap_delta(50)
                eng.set_lwwmap("reverse", 77)
            else:
                eng.set_lwwmap("reverse", 77)
                eng.set_lwwmap_delta(50)
            eng.tell(w.tells[0], w.tells[2])
            eng.run()
            out.append(eng.read_state()[0])
        finally:
            eng.close()
    assert np.array_equal(out[0], out[1])
    model = D.LwwDeltaModel(**w.engine_kwargs())
    w.apply_to(model)
    model.run()
    assert np.array_equal(out[0][:, :W], model.read_state()[0][:, :W])


def test_convergence_after_the_writers_stop(built):
    """Writer ticks, then ticks without writers plus gossip rounds: every key's replicas are equal, and every
    replica's delta_versions hold each peer's last seqNr, as in the model."""
    n = 40
    w = wl.crdt_lwwmap_delta(n, rounds=4, write=True, ops_per_replica=2, bucket_actors=32)
    ids = np.arange(n, dtype=np.uint32)

    def drive(t):
        t.run()
        t.tell(ids, np.full(n, Op.make(Op.DELTA_TICK, 7), np.uint32))
        t.tell(ids, np.full(n, Op.make(Op.GOSSIP, 11), np.uint32))
        return t.run()

    model = D.LwwDeltaModel(**w.engine_kwargs())
    w.apply_to(model)
    so = drive(model)
    assert model.key_converged()
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    try:
        w.apply_to(eng)
        sg = drive(eng)
        words = assert_same(eng, sg, model, so, "convergence")
    finally:
        eng.close()
    for g in range(0, n, 8):
        assert all(np.array_equal(words[a, :356], words[g, :356]) for a in range(g, min(g + 8, n)))
    for a in range(n):
        dec = DecodedMap.from_words(words[a])
        assert dec.delta_versions == tuple(model.dv[a]) and dec.entries == model.maps[a].entries
        assert all(dec.delta_versions[x % 8] == model.ctr[x] for x in range(a & ~7, min((a & ~7) + 8, n)) if x != a)
