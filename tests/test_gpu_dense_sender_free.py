"""The dense launches' sender-free inbox (agx_device.h km_reads_sender): a launch specialised to
RING -- whose behaviour cannot read its message's sender -- neither loads nor places the inbox's
sender array and never loads state word 1.  Every case is bit-exact against the BSP
oracle (counters, every state word, alive flags), at the smallest shapes at which each touched
branch can go wrong: one bucket +- 1 actor, a partial last bucket, the wrap-around tell into bucket
0; ring strides that keep a bucket's tells in its own bucket plus one neighbour (1), make every
tell foreign under one digit (2048), spread them over two foreign digits (3000: group_tells) and
sort the foreign run first (n - 1).  Hop budgets differ from actor to actor, so tokens die in
different supersteps and later inboxes are dense but not full."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd.engine import EngineConfig, GpuEngine, Kind, NO_SENDER, owner
from tests.test_gpu_parity import COUNT_KEYS, assert_same, run_both

pytestmark = pytest.mark.gpu

BUDGETS = (5, 3, 1000)  # (replays of 4 + 1, 2 + 1 supersteps, then the rest)


def ring(n, stride, n_words=1):
    """A RING population with one token per actor, hop budget 1 + (i % 5), stride `stride`; with
    n_words = 2 every actor's word 1 starts at a value of its own."""
    ids = np.arange(n, dtype=np.uint32)
    init = None
    if n_words > 1:
        init = np.zeros((n, n_words), np.uint64)
        init[:, 1] = (ids.astype(np.uint64) << np.uint64(32)) | np.uint64(0xA5A50000) | (ids % 7).astype(np.uint64)
    return wl.Workload("token_ring", n, n_words, 1, 5, 0, [(0, n, Kind.RING, init)], ring_stride=stride,
                       tells=(ids, np.full(n, NO_SENDER, np.uint32), (1 + ids % 5).astype(np.uint32)))


def run_budgets(w, name):
    """The same workload in superstep budgets, compared with the oracle after each."""
    from oracle import BspOracle
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    ref = BspOracle(**w.engine_kwargs())
    w.apply_to(eng)
    w.apply_to(ref)
    for budget in BUDGETS:
        sg, so = eng.run(budget), ref.run(budget)
        assert_same(sg, so, eng.read_state(), ref.read_state(), f"{name} budget={budget}")
    assert sg.in_flight == 0
    eng.close()


def strides(n):
    return [1, 2048, 3000, n - 1]


@pytest.mark.parametrize("si", range(4))
@pytest.mark.parametrize("n", [2047, 2049, 4099, 3 * 2048 + 17])
def test_ring_fused_sender_free(built, monkeypatch, n, si):
    monkeypatch.setenv("AGX_DENSE_FUSED", "1")
    s = strides(n)[si]
    sg, so, a, b = run_both(ring(n, s))
    assert_same(sg, so, a, b, f"ring n={n} s={s}")
    assert sg.delivered == int((2 + np.arange(n) % 5).sum()) and sg.dead_letters == 0
    run_budgets(ring(n, s), f"ring n={n} s={s}")


@pytest.mark.parametrize("s", [1, 3000])
def test_ring_fused_two_words(built, monkeypatch, s):
    """Word 1 is never loaded by the RING launch: it must come back as initialised."""
    monkeypatch.setenv("AGX_DENSE_FUSED", "1")
    n = 4099
    w = ring(n, s, n_words=2)
    sg, so, a, b = run_both(w)
    assert_same(sg, so, a, b, f"ring W=2 s={s}")
    assert np.array_equal(a[0][:, 1], w.ranges[0][3][:, 1])
    run_budgets(ring(n, s, n_words=2), f"ring W=2 s={s}")


@pytest.mark.parametrize("env", [{"AGX_DENSE_FUSED": "1", "AGX_PERSIST": "1"}, {"AGX_DENSE_FUSED": "0"}],
                         ids=["persist", "block_path"])
def test_ring_persistent_and_block_path(built, monkeypatch, env):
    """The persistent instantiation (the same bucket lambda) and the block path, which reads the
    arenas -- senders included -- that earlier launches wrote."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sg, so, a, b = run_both(ring(4099, 1))
    assert_same(sg, so, a, b, f"ring {env}")
    run_budgets(ring(4099, 1), f"ring {env}")


@pytest.mark.parametrize("mode", [{}, {"AGX_RADIX_BITS": "3"}], ids=["fused", "bits3"])
@pytest.mark.parametrize("case", ["one_per_actor", "one_per_actor_compiled", "mixed"])
def test_sender_reading_kinds_still_fed(built, monkeypatch, case, mode):
    """The sender-reading variants (PingPong replies, compiled operands) through the dense launch,
    k_dense_fused and k_dense_apply: their senders still arrive, and every counter -- unhandled and
    dead letters included -- still adds up."""
    monkeypatch.setenv("AGX_DENSE_LAUNCH", "1")
    for k, v in mode.items():
        monkeypatch.setenv(k, v)
    w = {"one_per_actor": lambda: wl.one_per_actor(20_000, seed=11),
         "one_per_actor_compiled": lambda: wl.one_per_actor(20_000, seed=12, compiled_kinds=True),
         "mixed": lambda: wl.mixed(4096)}[case]()
    sg, so, a, b = run_both(w)
    assert_same(sg, so, a, b, f"{case} {mode}")
    assert sg.dead_letters > 0 and (sg.unhandled > 0 or case == "one_per_actor_compiled")


def test_ring_sharded_loopback_owner(built, monkeypatch):
    """The owner instantiation (k_dense_fused<kOwner>): a hash-sharded ring over two loopback ranks."""
    from oracle import BspOracle
    monkeypatch.setenv("AGX_DENSE_LAUNCH", "1")
    monkeypatch.setenv("AGX_DENSE_OWNER", "1")
    ranks = 2
    w = wl.token_ring(40_000, 9)
    engs = [GpuEngine(EngineConfig(n_ranks=ranks, rank=r, **w.gpu_kwargs())) for r in range(ranks)]
    for e in engs:
        w.apply_to(e)
    sg = GpuEngine.group_run(engs)
    ref = BspOracle(n_ranks=ranks, **w.engine_kwargs())
    w.apply_to(ref)
    so = ref.run()
    for k in COUNT_KEYS:
        if k != "supersteps":
            assert getattr(sg, k) == so[k], (k, getattr(sg, k), so[k])
    wo, ao = ref.read_state()
    wg, ag = np.zeros_like(wo), np.zeros_like(ao)
    own_of = np.array([owner(i, 1000, ranks) for i in range(w.n_actors)])
    for e in engs:
        st, al = e.read_state()
        own = own_of == e.cfg.rank
        wg[own], ag[own] = st[own], al[own]
        e.close()
    assert np.array_equal(wg, wo) and np.array_equal(ag, ao)
