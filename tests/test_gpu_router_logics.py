"""Consistent-hashing and random routing on the GPU (agx_set_router_logics): the HIP engine through the
C ABI against the model (tests/router_model.py), on the fused and the multi-pass pipelines, with graph replays and eager
launches.  Everything is compared bit for bit after every run: states, alive flags, kinds, every counter,
receptionist_info, router_info, listings, masks, the hash rings, and conservation.  Buckets of 64 actors; 200 actors
are four buckets, the last partial; the static ring's segments hold 1024 points, so 200 x 13 points are two whole
segments and a partial one and 1000 x 5 four and a partial one."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import EngineConfig, GpuEngine
from tests.router_model import ConsistentHashRing, RouterModel

pytestmark = pytest.mark.gpu

B = typed.Behaviors
ctx = typed.context
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
TAGS = dict(Reg=1, Dereg=2, Stop=3, RouteH=4, RouteHN=5, RouteW=6, RouteI=7, RouteR=8, Work=9, Ack=10)
HASHED, PLAIN = typed.ServiceKey("hashed"), typed.ServiceKey("plain")
BIG = (1 << 32) * 5  # every actor's state word 0 starts above 2^32: RouteW hashes its low 32 bits
SEED = 0x5EED


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the receptionist fixture)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


@pytest.fixture(params=["replays", "eager"])
def launch(request, monkeypatch):
    if request.param == "eager":
        monkeypatch.setenv("AGX_NO_GRAPH", "1")
    return request.param


def pay(name: str, arg: int = 0) -> int:
    return (TAGS[name] << 24) | (arg & 0xFFFFFF)


def node_behavior() -> typed.Behavior:
    """Every actor of the scenarios.  Reg(k) / Dereg(k): key k (0: the hashed key, 1: the plain one); Stop.  RouteH(x):
    a hashed forward of Work(x) through key 0 keyed by x; RouteHN(x): the same, not a forward; RouteW: keyed by state
    word 0 (above 2^32); RouteI(x): by index through key 1; RouteR(x): a random forward of Work(x) through key 1 with
    the counter in state word 0.  Work(x) adds x + 1 to state word 1 and answers its sender Ack(x): a forward's sender
    is the host's NO_SENDER (a dead letter), a plain route's the router, which adds 2^20."""
    st = typed.State("cursor", "done")
    work, ack = typed.MessageType("Work", TAGS["Work"]), typed.MessageType("Ack", TAGS["Ack"])
    is_ = lambda t: (lambda m: m.tag == TAGS[t])
    rb = typed.ReceiveBuilder.create(st)
    rb.on_any_message(lambda m, s: [B.stopped], test=is_("Stop"))
    rb.on_any_message(lambda m, s: [s.done.add(m.arg + 1), m.sender.tell(ack(m.arg)), B.same], test=is_("Work"))
    rb.on_any_message(lambda m, s: [s.done.add(1 << 20), B.same], test=is_("Ack"))
    rb.on_any_message(lambda m, s: [ctx.route_hashed(HASHED, m.arg, work(m.arg)), B.same], test=is_("RouteH"))
    rb.on_any_message(lambda m, s: [ctx.route_hashed(HASHED, m.arg, work(m.arg), forward=False), B.same], test=is_("RouteHN"))
    rb.on_any_message(lambda m, s: [ctx.route_hashed(HASHED, s.cursor, work(m.arg)), B.same], test=is_("RouteW"))
    rb.on_any_message(lambda m, s: [ctx.route_by(PLAIN, m.arg, work(m.arg)), B.same], test=is_("RouteI"))
    rb.on_any_message(lambda m, s: [ctx.route_random(PLAIN, work(m.arg), counter=s.cursor), B.same], test=is_("RouteR"))
    for k, key in enumerate((HASHED, PLAIN)):
        arg = (lambda k: (lambda m, s: m.arg == k))(k)
        rb.on_any_message((lambda key: lambda m, s: [ctx.register(key), B.same])(key), test=is_("Reg"), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [ctx.deregister(key), B.same])(key), test=is_("Dereg"), when=arg)
    rb.on_any_message(lambda m, s: [B.unhandled])
    return rb.build("router_node")


def node_workload(n: int, factor: int, starts=(), T: int = 3) -> wl.Workload:
    node = node_behavior()
    tb = typed.compile_behaviors([node], max_emit=1)
    assert tb.service_keys == [HASHED, PLAIN] and tb.hashed_keys == [0]
    init = np.zeros((n, 2), np.uint64)
    init[:, 0] = BIG + np.arange(n, dtype=np.uint64) * 7
    return wl.Workload("router_nodes", n, 2, 1, T, 0, [(0, n, tb.kind_of(node), init)], behaviors=tb, bucket_actors=64,
                       receptionist={"n_keys": 2, "capacity": n, "starts": list(starts)},
                       router_logics={"hashed_keys_mask": 1, "virtual_nodes_factor": factor, "seed": SEED})


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def model_for(w):
    m = RouterModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def snapshot(t, n_keys: int, hashed=(0,)) -> dict:
    words, alive = t.read_state()
    d = dict(words=np.asarray(words).tolist(), alive=(np.asarray(alive) & 1).tolist(), kinds=np.asarray(t.read_kinds()).tolist(),
             info=t.receptionist_info(), router_info=t.router_info(), masks=t.read_services().tolist(),
             listings=[t.read_listing(k).tolist() for k in range(n_keys)])
    for k in hashed:
        hs, ids = t.read_hash_ring(k)
        d[f"ring{k}"] = [np.asarray(hs).tolist(), np.asarray(ids).tolist()]
    return d


def both(w, script, n_keys=2, hashed=(0,)):
    """run `script(target)` -- a generator that yields every run's stats -- on the engine and the model and compare
    everything after every run; the last stats and the last snapshot"""
    eng, mod = engine_for(w), model_for(w)
    n, sm, m = 0, None, None
    for sg, sm in zip(script(eng), script(mod)):
        sg, sm = counts(sg), counts(sm)
        assert sg == sm, (n, sg, sm)
        g, m = snapshot(eng, n_keys, hashed), snapshot(mod, n_keys, hashed)
        for k in g:
            assert g[k] == m[k], (n, k)
        assert sg["staged"] + sg["emitted"] == sg["delivered"] + sg["dead_letters"] + sg["in_flight"]
        n += 1
    eng.close()
    return sm, m


def tell(t, *msgs):
    """(dst, payload) ... from the host"""
    t.tell(np.asarray([d for d, _ in msgs], np.uint32), np.asarray([p for _, p in msgs], np.uint32))


HASH_KEYS = (0, 9, 10, (1 << 24) - 1)
SIZES = [(200, 1), (200, 2), (200, 13), (1000, 5)]


def workers_of(n):
    """the hashed key's setup members: every third actor from 1 on, in every bucket"""
    return list(range(1, n, 3))


def starts_of(n):
    return [(a, 1, 0) for a in workers_of(n)] + [(n // 2, n // 4, 1)]


# ------------------------------------------------------------------ 1. a static pool, the hash keys of the issue
@pytest.mark.parametrize("n,factor", SIZES)
def test_static_pool(built, pipeline, launch, n, factor):
    w = node_workload(n, factor, starts_of(n))

    def script(t):
        yield t.run()  # (nothing staged: the rings of the setup block)
        tell(t, *[(r, pay("RouteH", x)) for r in (0, 63, 64, n - 1) for x in HASH_KEYS],
             *[(2, pay("RouteHN", x)) for x in HASH_KEYS], (5, pay("RouteW", 3)), (n - 2, pay("RouteW", 4)),
             *[(7, pay("RouteI", x)) for x in range(5)], *[(8, pay("RouteR", x)) for x in range(5)])
        yield t.run()
    st, snap = both(w, script)
    ring = ConsistentHashRing(workers_of(n), factor)
    assert snap["ring0"][1] == ring.ids().tolist() and len(snap["ring0"][1]) == factor * len(workers_of(n))
    assert snap["router_info"] == dict(hashed=4 * 4 + 4 + 2, random=5, ring_rebuilds=0, ring_size=[len(ring)] + [0] * 7)
    # where the low-32-bits rule and the forwards put the work: expected from the ring alone
    done = np.zeros(n, np.int64)
    for x in HASH_KEYS:
        done[ring.node_for(str(x))] += 5 * (x + 1)          # four forwards and one plain route
    done[2] += 4 << 20                                      # the plain routes' Acks come back to the router
    done[ring.node_for(str((BIG + 5 * 7) & 0xFFFFFFFF))] += 4
    done[ring.node_for(str((BIG + (n - 2) * 7) & 0xFFFFFFFF))] += 5
    hashed_part = np.asarray(snap["words"])[:, 1].astype(np.int64)
    plain = set(range(n // 2, n // 2 + n // 4))
    for a in range(n):
        if a not in plain:
            assert hashed_part[a] == done[a], a
    assert st["dead_letters"] == 4 * 4 + 2 + 5 + 5  # the forwards' Acks to NO_SENDER


# ------------------------------------------------------------------ 2. workers that deregister, stop and register mid-run
@pytest.mark.parametrize("n,factor", SIZES)
def test_a_changing_pool(built, pipeline, launch, n, factor):
    w = node_workload(n, factor, starts_of(n))
    ws = workers_of(n)
    routes = lambda t, r0: tell(t, *[(r0 + i, pay("RouteH", 100 + i)) for i in range(40)])

    def script(t):
        routes(t, 0)
        tell(t, (ws[0], pay("Dereg", 0)), (ws[-1], pay("Stop")), (ws[5], pay("Stop")))
        yield t.run(1)  # the routes of this tick still see the old ring ...
        routes(t, 0)
        yield t.run(1)  # ... those of the next the new one; the stopped actors' mail is dead
        tell(t, (0, pay("Reg", 0)), (n - 2, pay("Reg", 0)), (ws[0], pay("Reg", 0)), (64, pay("Reg", 1)))
        routes(t, 40)
        yield t.run(1)
        routes(t, 40)
        yield t.run()
    st, snap = both(w, script)
    members = sorted(set(ws) - {ws[-1], ws[5]} | {0, n - 2})
    assert sorted(set(snap["ring0"][1])) == members and snap["listings"][0] == members
    assert snap["router_info"]["ring_rebuilds"] == 2 and snap["router_info"]["ring_size"][0] == factor * len(members)
    assert snap["info"]["terminated"] == 2 and snap["info"]["rebuilds"] == len(starts_of(n)) + 3  # (key 1 once)


# ------------------------------------------------------------------ 3. a ring emptied and refilled
def test_a_ring_emptied_and_refilled(built, pipeline, launch):
    n = 200
    w = node_workload(n, 2, [(10, 1, 0), (70, 1, 0), (199, 1, 0)])

    def script(t):
        tell(t, (10, pay("Dereg", 0)), (70, pay("Stop")), (199, pay("Dereg", 0)), (3, pay("RouteH", 9)))
        yield t.run()
        tell(t, (3, pay("RouteH", 9)), (4, pay("RouteHN", 10)), (5, pay("RouteW")))  # an empty ring: dead letters
        yield t.run()
        tell(t, (130, pay("Reg", 0)))
        yield t.run()
        tell(t, (3, pay("RouteH", 9)), (4, pay("RouteHN", 10)))
        yield t.run()
    st, snap = both(w, script)
    assert snap["ring0"][1] == [130, 130]
    assert snap["info"]["no_routees"] == 3 and snap["router_info"]["hashed"] == 3
    assert snap["words"][130][1] == 10 + 11 and snap["words"][4][1] == 1 << 20


# ------------------------------------------------------------------ 4. agx_register_services between runs
def test_register_services_between_runs(built, pipeline, launch):
    n = 200
    w = node_workload(n, 13, [(60, 10, 0)])

    def script(t):
        tell(t, *[(i, pay("RouteH", i)) for i in range(30)])
        yield t.run()
        t.register_services(0, n, 0, True)      # everybody: 2600 points
        t.register_services(64, 64, 0, False)   # a whole bucket leaves
        yield t.run()                           # (nothing staged: the rings alone)
        tell(t, *[(i, pay("RouteH", i)) for i in range(30)])
        yield t.run()
        t.register_services(0, n, 0, False)     # emptied by the host
        tell(t, (1, pay("RouteH", 1)))
        yield t.run()
    st, snap = both(w, script)
    assert snap["router_info"]["ring_rebuilds"] == 3 and snap["router_info"]["ring_size"][0] == 0
    assert snap["info"]["no_routees"] == 1


# ------------------------------------------------------------------ 5. random routing over a changing listing
def test_random_routing_over_a_changing_listing(built, pipeline, launch):
    n = 200
    w = node_workload(n, 1, [(100, 50, 1)])

    def script(t):
        for tick in range(6):
            tell(t, *[(r, pay("RouteR", tick)) for r in (0, 1, 63, 64, 199)],
                 *([(100 + 7 * tick, pay("Stop")), (110 + tick, pay("Dereg", 1)), (20 + tick, pay("Reg", 1))]))
            yield t.run(1)
        yield t.run()
        t.register_services(0, n, 1, False)
        tell(t, (0, pay("RouteR", 1)))
        yield t.run()
    st, snap = both(w, script)
    assert snap["router_info"]["random"] == 30 and snap["info"]["no_routees"] == 1
    assert snap["words"][0][0] == BIG + 6  # the counter moved once per hit and not on the miss


# ------------------------------------------------------------------ 6. the seeded mesh: everything at once
@pytest.mark.parametrize("n,factor", SIZES)
def test_mesh(built, pipeline, n, factor):
    w = node_workload(n, factor, starts_of(n), T=2)
    rng = np.random.default_rng(n * 100 + factor)
    plan = []
    for tick in range(10):
        msgs = []
        for name, cnt in (("RouteH", 24), ("RouteHN", 6), ("RouteW", 4), ("RouteI", 6), ("RouteR", 10), ("Reg", 5), ("Dereg", 4),
                          ("Stop", 2)):
            for a in rng.integers(0, n, cnt).tolist():
                arg = int(rng.integers(0, 2)) if name in ("Reg", "Dereg") else int(rng.integers(0, 1 << 24))
                msgs.append((a, pay(name, arg)))
        plan.append(msgs)

    def script(t):
        for msgs in plan:
            tell(t, *msgs)
            yield t.run(1)
        yield t.run()
    st, snap = both(w, script)
    ri = snap["router_info"]
    assert ri["hashed"] > 200 and ri["random"] > 50 and ri["ring_rebuilds"] >= 8


# ------------------------------------------------------------------ 7. both workloads at toy size
def run_workload(w, hashed):
    def script(t):
        for dst, src, py in w.schedule:
            t.tell(dst, py, src)
            yield t.run(1)
        yield t.run()
    return both(w, script, n_keys=1, hashed=hashed)


def test_sticky_sessions(built, pipeline, launch):
    w = wl.sticky_sessions(n_clients=256, n_routers=8, n_workers=64, n_spare=8, quota=5, virtual_nodes_factor=10, ticks=8,
                           join_at=3, seed=3, bucket_actors=64)
    st, snap = run_workload(w, (0,))
    ri = snap["router_info"]
    assert ri["hashed"] + snap["info"]["no_routees"] == 256 * 8 and ri["ring_rebuilds"] >= 5
    assert snap["info"]["terminated"] > 0 and st["in_flight"] == 0


def test_random_pool(built, pipeline, launch):
    w = wl.random_pool(n_routers=100, n_workers=150, ticks=8, quota=4, seed=4, bucket_actors=64)
    st, snap = run_workload(w, ())
    assert snap["router_info"]["random"] + snap["info"]["no_routees"] == 800 and snap["info"]["terminated"] > 100
    assert snap["router_info"]["ring_size"] == [0] * 8 and snap["router_info"]["hashed"] == 0
