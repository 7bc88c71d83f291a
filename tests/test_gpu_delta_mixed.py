"""GPU parity of delta-CRDT replication with more than one data type in the engine (the V_ALL_DELTA
apply variant): GCounter, ORSet and PNCounter replicas share one row heap at the ORSet pitch, and
throughput caps keep the DeltaPropagations of every type waiting in the mailboxes, where
k_bucket_apply copies a queued row forward each superstep.  The HIP engine through the C ABI vs the
BSP oracle, bit-exact on every counter and every state word (data, deltaVersions, selector state
and delta log) -- and with the row heap poisoned (AGX_HEAP_POISON), so that a row word which the
reader reads and no writer wrote gives the same failure on every run, whatever the allocator
returns.

Every case also checks its own premises on the reference run: the census of queued
DeltaPropagations (BspOracle.delta_backlog_census) shows that counter rows did wait in mailboxes,
the misaligned cases delivered groups to replicas of another type, and with `big` counters the
high u32 half of a counter slot of every counter replica is in use."""
import functools

import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd.engine import EngineConfig, GpuEngine, Kind, owner
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

POISON = [None, "0", "255"]
IDS = ["unset", "p0", "p255"]


def make(spec):
    kw = dict(spec)
    if "orset_only" in kw:  # the single-kind workload (the V_OR_DELTA variant)
        return wl.crdt_delta(kw.pop("orset_only"), Kind.ORSET, **kw)
    return wl.crdt_delta_mixed(**kw)


@functools.lru_cache(maxsize=None)
def reference(spec, ranks=1):
    """One BSP oracle run per case, shared by its poison values: (stats, (words, alive), census).
    The arrays are read-only from here on."""
    from oracle import BspOracle
    w = make(spec)
    ref = BspOracle(n_ranks=ranks, **w.engine_kwargs())
    w.apply_to(ref)
    so = ref.run()
    wo, ao = ref.read_state()
    census = ref.delta_backlog_census()
    ref.close()
    wo.setflags(write=False)
    ao.setflags(write=False)
    return so, (wo, ao), census


def set_poison(monkeypatch, poison):
    if poison is None:
        monkeypatch.delenv("AGX_HEAP_POISON", raising=False)
    else:
        monkeypatch.setenv("AGX_HEAP_POISON", poison)


def check_premises(spec, so, sto, census, min_queued, cross_kind=False):
    """The reference run itself exercised what the case is about."""
    assert so["in_flight"] == 0
    print(f"census {census} unhandled {so['unhandled']}")
    assert census[0] >= min_queued and census[1] >= min_queued, f"counter rows did not queue: {census}"
    if cross_kind:
        assert so["unhandled"] > 0, "no group reached a replica of another data type"
    kw = dict(spec)
    if kw.get("big", True):
        c0, c1, c2 = kw.get("counts", (320, 320, 320))
        words = sto[0]
        assert (words[:c0, :8] >= 1 << 32).any(axis=1).all()                       # GCounter replicas
        assert (words[c0 + c1:c0 + c1 + c2, :16] >= 1 << 32).any(axis=1).all()     # PNCounter replicas


def run_case(monkeypatch, poison, spec, min_queued, name, cross_kind=False):
    """run_both / assert_same of tests/test_gpu_parity.py, with the reference run shared between the
    poison values of a case and its census read."""
    set_poison(monkeypatch, poison)
    so, sto, census = reference(spec)
    check_premises(spec, so, sto, census, min_queued, cross_kind)
    w = make(spec)
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    w.apply_to(eng)
    sg = eng.run()
    stg = eng.read_state()
    eng.close()
    assert_same(sg, so, stg, sto, f"{name} poison={poison}")


def spec_of(**kw):
    return tuple(sorted(kw.items()))


# Census of the reference (GCounter, PNCounter, ORSet) at counts (320, 320, 320), rounds 8:
#   T=1 C=0 M=2:  (14080, 14080, 3371)     T=2 C=6 M=50: (4680, 4680, 4680)
#   T=1 C=0 M=50: (14080, 14080, 14080)    T=5 C=0 M=50: (1040, 1040, 1040)
# The T=5 case asserts half of what the reference gives; the others 1000, far below it.
QUEUED_T5 = 520


@pytest.mark.parametrize("poison", POISON, ids=IDS)
@pytest.mark.parametrize("T,C,M,min_queued", [(1, 0, 2, 1000), (2, 6, 50, 1000), (1, 0, 50, 1000), (5, 0, 50, QUEUED_T5)])
def test_mixed_queued_rows_pure_delta(built, monkeypatch, poison, T, C, M, min_queued):
    """No full-state gossip: nothing heals a DeltaPropagation that a forward copy lost."""
    spec = spec_of(throughput=T, capacity=C, max_delta_size=M, gossip_rounds=0)
    run_case(monkeypatch, poison, spec, min_queued, f"mixed delta T={T} C={C} M={M}")


@pytest.mark.parametrize("poison", POISON, ids=IDS)
def test_mixed_queued_rows_with_gossip(built, monkeypatch, poison):
    """Full-state gossips (rows at the full ORSet length) queue beside the DeltaPropagations."""
    spec = spec_of(throughput=3, gossip_rounds=2)
    run_case(monkeypatch, poison, spec, 1000, "mixed delta gossip T=3")


@pytest.mark.parametrize("poison", POISON, ids=IDS)
@pytest.mark.parametrize("T,M,G", [(1, 50, 0), (3, 2, 2)])
def test_mixed_misaligned_ranges(built, monkeypatch, poison, T, M, G):
    """Range sizes that are no multiple of 8: two keys straddle a boundary between data types (a
    counter group reaches an ORSet replica and the other way round: Behaviors.unhandled), and the
    last key has fewer than 8 replicas."""
    spec = spec_of(counts=(323, 322, 321), throughput=T, max_delta_size=M, gossip_rounds=G)
    run_case(monkeypatch, poison, spec, 1000, f"mixed delta misaligned T={T} M={M} G={G}", cross_kind=True)


@pytest.mark.parametrize("poison", POISON, ids=IDS)
def test_mixed_with_plain_actors(built, monkeypatch, poison):
    """COUNTER actors after the replicas: the kinds mask also holds a non-CRDT kind."""
    spec = spec_of(plain=64)
    run_case(monkeypatch, poison, spec, 1000, "mixed delta plain=64")


@pytest.mark.parametrize("poison", POISON, ids=IDS)
def test_mixed_smallest_population(built, monkeypatch, poison):
    """192 replicas: one bucket."""
    spec = spec_of(counts=(64, 64, 64), throughput=1)
    run_case(monkeypatch, poison, spec, 200, "mixed delta 3x64")


@pytest.mark.parametrize("poison", POISON, ids=IDS)
def test_mixed_zero_initialised_counters(built, monkeypatch, poison):
    """Counter values near 0 (the other cases start the counters above 2^40)."""
    spec = spec_of(big=False)
    run_case(monkeypatch, poison, spec, 1000, "mixed delta big=False")


@pytest.mark.parametrize("poison", POISON, ids=IDS)
@pytest.mark.parametrize("ba", [32, 512, 2048])
def test_mixed_bucket_widths(built, monkeypatch, poison, ba):
    spec = spec_of(throughput=2, bucket_actors=ba)
    run_case(monkeypatch, poison, spec, 1000, f"mixed delta ba={ba}")


@pytest.mark.parametrize("poison", POISON, ids=IDS)
def test_mixed_skew_path(built, monkeypatch, poison):
    """A 2048-replica bucket with more than one 2048-message tile: the skew launch."""
    spec = spec_of(counts=(704, 704, 704), bucket_actors=2048, throughput=5)
    run_case(monkeypatch, poison, spec, 1000, "mixed delta skew")  # (reference: 2288, 2288, 239)


@pytest.mark.parametrize("poison", POISON, ids=IDS)
def test_mixed_multipass(built, monkeypatch, poison):
    monkeypatch.setenv("AGX_RADIX_BITS", "3")
    spec = spec_of(counts=(323, 322, 321))
    run_case(monkeypatch, poison, spec, 1000, "mixed delta multipass", cross_kind=True)


@pytest.mark.parametrize("poison", POISON, ids=IDS)
@pytest.mark.parametrize("ranks", [2, 3])
def test_mixed_loopback_sharded(built, monkeypatch, poison, ranks):
    """Hash-sharded replicas: rows of every data type cross the rank slabs, with the row buffers of
    the exchange poisoned too."""
    set_poison(monkeypatch, poison)
    spec = spec_of(counts=(160, 160, 160), throughput=2)
    so, (wo, _), census = reference(spec, ranks)
    check_premises(spec, so, (wo, None), census, 1000)  # (reference: 2568, 2562, 562 / 2557, 2561, 531)
    w = make(spec)
    engs = [GpuEngine(EngineConfig(n_ranks=ranks, rank=r, **w.gpu_kwargs())) for r in range(ranks)]
    for e in engs:
        w.apply_to(e)
    sg = GpuEngine.group_run(engs)
    for k in ("delivered", "dead_letters", "unhandled", "emitted", "staged", "in_flight"):
        assert getattr(sg, k) == so[k], (k, getattr(sg, k), so[k])
    wg = np.zeros_like(wo)
    own_of = np.array([owner(i, 1000, ranks) for i in range(w.n_actors)])
    for e in engs:
        a, _ = e.read_state()
        own = own_of == e.cfg.rank
        wg[own] = a[own]
        e.close()
    diff = np.nonzero((wg != wo).any(axis=1))[0]
    assert diff.size == 0, diff[:10]


def test_mixed_rows_recycled(built, monkeypatch):
    """40 rounds at throughput 1 without poison: every heap row is reused many times, by counter
    groups and by ORSet groups (the state a real run leaves in a recycled row)."""
    spec = spec_of(counts=(64, 64, 64), rounds=40, throughput=1)
    run_case(monkeypatch, None, spec, 200, "mixed delta recycled")


@pytest.mark.parametrize("poison", POISON, ids=IDS)
def test_orset_only_used_length_under_poison(built, monkeypatch, poison):
    """The one variant that copies a queued DeltaPropagation by its used length (V_OR_DELTA: every
    group is an ORSet group, whose writer stores the length in the row's last word), with the heap
    poisoned: full-state gossips (no length word, whole pitch) queue beside the groups, and the last
    key has 5 replicas.  The reference's census of ORSet groups is 56454 envelope-supersteps; half of that is asserted."""
    set_poison(monkeypatch, poison)
    spec = spec_of(orset_only=8 * 120 + 5, rounds=8, write=True, ops_per_replica=3, gossip_rounds=3, throughput=1,
                   max_delta_size=50, bucket_actors=512)
    so, sto, census = reference(spec)
    print(f"census {census}")
    assert census[0] == 0 and census[1] == 0 and census[2] >= 28227 and so["in_flight"] == 0
    w = make(spec)
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    w.apply_to(eng)
    sg = eng.run()
    stg = eng.read_state()
    eng.close()
    assert_same(sg, so, stg, sto, f"orset-only delta poison={poison}")
