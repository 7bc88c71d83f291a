"""The receptionist and group routers on the GPU (agx_set_receptionist): the HIP engine through the
C ABI against the known answers restated from the reference's specs (tests/golden/receptionist_kats.json) and
against the model (tests/receptionist_model.py), on the fused and the multi-pass pipelines, with graph replays and
eager launches.  Everything is compared bit for bit after every run: states, alive flags, kinds, every counter,
receptionist_info, read_listing, read_services, the outbox order, and conservation."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import NO_SENDER, EngineConfig, GpuEngine, Kind
from tests import receptionist_cases as rc
from tests.receptionist_model import ReceptionistModel

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = 1, 5, 6
B = typed.Behaviors
ctx = typed.context


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the death-watch fixture)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


@pytest.fixture(params=["replays", "eager"])
def launch(request, monkeypatch):
    if request.param == "eager":
        monkeypatch.setenv("AGX_NO_GRAPH", "1")
    return request.param


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def model_for(w):
    m = ReceptionistModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def refusal(call):
    """(status, message) of the refusal"""
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]


def conserved(st):
    return st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def both(w, script):
    """run `script(target)` -- a generator that yields after every run's stats -- on the engine and the model and
    compare everything after every run"""
    eng, mod = engine_for(w), model_for(w)
    nk = w.receptionist["n_keys"]
    n, sm, m = 0, None, None
    for sg, sm in zip(script(eng), script(mod)):
        sg, sm = rc.counts(sg), rc.counts(sm)
        assert sg == sm, (n, sg, sm)
        g, m = rc.snapshot(eng, nk), rc.snapshot(mod, nk)
        for k in g:
            assert g[k] == m[k], (n, k, g[k], m[k])
        assert conserved(sg)
        n += 1
    eng.close()
    return sm, m


# ------------------------------------------------------------------ 1. the known answers (64 actors, one bucket)
@pytest.mark.parametrize("T", rc.KAT_T)
@pytest.mark.parametrize("name", rc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(rc.kat_workload(name, T))
    got = rc.run_kat(name, T, eng)
    eng.close()
    print(got)
    rc.check_kat(name, got)
    assert got == rc.run_kat(name, T, model_for(rc.kat_workload(name, T)))


# ------------------------------------------------------------------ 2. four buckets of 64: the wave and bucket edges
@pytest.mark.parametrize("T", [1, 3])
def test_edges_of_four_buckets(built, pipeline, launch, T):
    """members at local indices 0, 63 and 64, the last actor, no member in bucket 2 between two buckets with
    members; keys 0 and n_keys - 1; all 8 keys dirty in one tick; router and routee in one bucket and in two"""
    w = rc.node_workload(T, n=256, n_keys=8)
    members = (0, 63, 64, 255)

    def script(t):
        rc.tells(t, *[(a, "Reg:0") for a in members], *[(a, "Reg:7") for a in members])
        yield t.run()
        rc.tells(t, *[(1, f"Route:{i}") for i in range(5)], *[(200, f"Route:{i}") for i in range(3)],
                 (70, "RouteBy:6"), (1, "Size:7"), (1, "At:3"))
        yield t.run()
        rc.tells(t, *[(100 + k, f"Reg:{k}") for k in range(8)], (63, "Dereg:7"), (64, "Stop"))  # every key in one tick
        yield t.run(1)
        yield t.run()
        rc.tells(t, *[(130 + k, f"Reg:{k}") for k in range(8)])  # members in bucket 2 after all
        yield t.run()
    st, snap = both(w, script)
    assert snap["listings"][0] == [0, 63, 100, 130, 255] and snap["listings"][7] == [0, 107, 137, 255]
    assert snap["info"]["terminated"] == 2 and snap["info"]["routed"] == 9 and snap["info"]["size"][3] == 2


# ------------------------------------------------------------------ 3. the capacity of a listing
def test_listing_of_exactly_capacity_then_one_more(built, pipeline):
    w = rc.node_workload(3, n=256, listing_capacity=5)
    eng = engine_for(w)
    rc.tells(eng, *[(a, "Reg:0") for a in (3, 70, 130, 200, 255)])
    eng.run()
    assert eng.read_listing(0).tolist() == [3, 70, 130, 200, 255]  # exactly `capacity` ids: no error
    rc.tells(eng, (64, "Reg:0"))
    text = ("a service key's listing would hold more than 5 ids, the receptionist's capacity (agx_set_receptionist): the "
            "listing keeps its first 5 ids")
    assert refusal(eng.run) == (ECAPACITY, text)
    assert refusal(eng.run) == (ECAPACITY, text)  # sticky
    assert eng.read_listing(0).tolist() == [3, 64, 70, 130, 200]
    eng.close()


# ------------------------------------------------------------------ 4. a routee that stops in the tick it is routed to
def test_routee_stops_in_the_tick_it_is_routed_to(built, pipeline, launch):
    w = rc.node_workload(3, n=256, starts=[(70, 1, 0), (200, 1, 0)])

    def script(t):
        rc.tells(t, (1, "Route:1"))  # tick 1: routed to 70 ...
        yield t.run(1)
        rc.tells(t, (70, "Stop"))    # ... which handles it in tick 2, before the Stop staged behind it
        yield t.run(1)
        yield t.run()
        rc.tells(t, (1, "Route:2"))
        yield t.run()
    st, snap = both(w, script)
    assert snap["alive"][70] == 0 and snap["listings"][0] == [200] and snap["info"]["terminated"] == 1


def test_mail_of_a_stopped_routee_is_dead_letters(built, pipeline):
    """70 stops in tick 1; the Work routed to it in tick 1 arrives in tick 2 as a dead letter, and the listing of
    tick 2 lacks it: the next route goes to 200"""
    w = rc.node_workload(3, n=256, starts=[(70, 1, 0), (200, 1, 0)])

    def script(t):
        rc.tells(t, (70, "Stop"), (1, "Route:1"))
        yield t.run(1)
        rc.tells(t, (1, "Route:2"))
        yield t.run()
    st, snap = both(w, script)
    assert st["dead_letters"] == 1 and snap["words"][200][1] == 1 and snap["listings"][0] == [200]


# ------------------------------------------------------------------ 5. the version counts net changes
def test_register_and_deregister_in_one_window(built, pipeline, launch):
    w = rc.node_workload(3, n=256)

    def script(t):
        rc.tells(t, (65, "Reg:1"), (65, "Dereg:1"), (65, "Reg:0"), (190, "Reg:0"), (190, "Stop"))
        yield t.run()
    st, snap = both(w, script)
    i = snap["info"]
    assert (i["version"][:2], i["rebuilds"], i["registered"], i["deregistered"], i["terminated"]) == ([1, 0], 1, 3, 1, 1)
    assert snap["listings"] == [[65], []]


# ------------------------------------------------------------------ 6. a run that ends on a tick with changes; the setup block between runs
def test_run_ends_on_a_tick_with_changes_and_register_services_between_runs(built, pipeline, launch):
    w = rc.node_workload(1, n=256)

    def script(t):
        rc.tells(t, (5, "Reg:0"), (5, "Reg:1"), (250, "Reg:0"))
        yield t.run(1)  # (T = 1: actor 5's second message waits; the run ends on a tick that changed key 0)
        yield t.run()
        t.register_services(60, 10, 0)          # 60..69: two buckets
        t.register_services(0, 256, 1, False)   # everyone leaves key 1
        yield t.run()                           # (no mail: the listings are in force all the same)
        rc.tells(t, *[(1, f"Route:{i}") for i in range(4)])
        yield t.run()
        t.register_services(62, 2, 0, False)
        yield t.run()
    st, snap = both(w, script)
    assert snap["listings"] == [[5, 60, 61] + list(range(64, 70)) + [250], []]
    assert snap["info"]["version"][:2] == [3, 2]


# ------------------------------------------------------------------ 7. a forward from a host-side sender
def test_forward_from_a_host_side_sender(built, pipeline, launch):
    """Routers.group forwards: the job's sender (a host-side actor, the replyTo) stays on the routed envelope and
    the worker's reply reaches the outbox"""
    w = wl.service_pool(8, 120, ticks=6, quota=3, n_host=2, bucket_actors=64)

    replies = []  # the outbox of the third tick, of the engine and of the model: senders (workers), host ids, payloads

    def script(t):
        for i, (dst, src, pay) in enumerate(w.schedule):
            t.tell(dst, pay, src)
            st = t.run(1)
            if i == 2:
                d, s, p = t.take_outbound()
                replies.append((sorted(s.tolist()), sorted(d.tolist()), sorted(p.tolist())))
            yield st
        yield t.run()
    st, snap = both(w, script)
    assert len(replies) == 2 and replies[0] == replies[1] and len(replies[0][0]) == 8  # (the third tick: the 8 jobs routed in the second)
    assert snap["info"]["routed"] > 0 and replies and all(set(r[1]) <= {128, 129} for r in replies)
    assert 0 < snap["info"]["size"][0] < 120 and snap["info"]["terminated"] == 120 - snap["info"]["size"][0]


def test_plain_forward_and_route_without_forward(built, pipeline):
    """ref.forward(msg) on a plain tell keeps the sender; route(forward=False) makes the router the sender"""
    key = typed.ServiceKey("k")
    st = typed.State("cursor", "n")
    node = (typed.ReceiveBuilder.create(st)
            .on_any_message(lambda m, s: [typed.self_ref(1).forward(m.arg + 1), B.same], test=lambda m: m.tag == 1)
            .on_any_message(lambda m, s: [ctx.route(key, m.arg + 1, cursor=s.cursor, forward=False), B.same],
                            test=lambda m: m.tag == 2)
            .on_any_message(lambda m, s: [s.n.inc(), m.sender.tell(m.payload), B.same], test=lambda m: m.sender.dst >= 128)
            .on_any_message(lambda m, s: [s.n.inc(), B.same])
            .build("fwd"))
    tb = typed.compile_behaviors([node], max_emit=1)
    assert tb.uses_forward and tb.uses_receptionist
    w = wl.Workload("fwd", 128, 2, 1, 3, 0, [(0, 128, tb.kind_of(node), None)], behaviors=tb, bucket_actors=64,
                    outbound=(128, 1), receptionist={"n_keys": 1, "capacity": 128, "starts": [(100, 1, 0)]})

    def script(t):
        t.tell(np.asarray([63, 5], np.uint32), np.asarray([(1 << 24) | 7, (2 << 24) | 9], np.uint32), np.asarray([128, 128], np.uint32))
        yield t.run()
    st, snap = both(w, script)
    # 63 forwards to 64, which sees the host as the sender and answers it; 5 routes to 100, which sees the router
    assert snap["outbox"] == [[64], [128], [8]] and snap["words"][100][1] == 1 and snap["words"][5][0] == 101


# ------------------------------------------------------------------ 8. the differential workload
def test_service_mesh_4096(built, pipeline):
    w = wl.service_mesh(4096, n_keys=8, seed=3, ticks=40)
    eng, mod = engine_for(w), model_for(w)
    for t, (dst, src, pay) in enumerate(w.schedule):
        for x in (eng, mod):
            x.tell(dst, pay, src)
        sg, sm = rc.counts(eng.run(1)), rc.counts(mod.run(1))
        assert sg == sm, (t, sg, sm)
        if t % 8 == 7:
            assert eng.receptionist_info() == mod.receptionist_info(), t
    sg, sm = rc.counts(eng.run()), rc.counts(mod.run())
    assert sg == sm and conserved(sg)
    g, m = rc.snapshot(eng, 8), rc.snapshot(mod, 8)
    eng.close()
    for k in g:
        assert g[k] == m[k], k
    assert mod.max_bucket_inbox(64) <= 2048 and min(m["info"]["version"]) > 10 and m["info"]["terminated"] > 0


# ------------------------------------------------------------------ 9. one tile per bucket
def test_a_bucket_over_one_tile_is_loud(built, pipeline):
    eng = engine_for(rc.node_workload(3, n=128))
    eng.tell(np.arange(2100, dtype=np.uint32) % 64, np.full(2100, rc.payload("Work:1"), np.uint32),
             np.full(2100, NO_SENDER, np.uint32))
    st, text = refusal(eng.run)
    eng.close()
    assert st == ECAPACITY and text == (
        "a bucket of 64 actors of an engine with the receptionist received more than one tile of 2048 messages (backlog "
        "included): the launches for larger inboxes know no receptionist (smaller agx_cfg.bucket_actors spread the load)")


# ------------------------------------------------------------------ 10. every refusal, status and text
def plain_engine(registered=64, **cfg):
    eng = GpuEngine(EngineConfig(**dict(dict(n_actors=64, bucket_actors=32, throughput=3, capacity=0, n_words=2, max_emit=1),
                                        **cfg)))
    eng.register_range(0, registered, Kind.COUNTER)
    eng.set_mailbox_class(1, 0)
    return eng


def test_argument_checks_and_second_call(built):
    eng = plain_engine()
    assert refusal(lambda: eng.set_receptionist(0, 4)) == (EINVAL, "the receptionist: 0 service keys (1..8), listings of 4 ids (at least 1)")
    assert refusal(lambda: eng.set_receptionist(9, 4)) == (EINVAL, "the receptionist: 9 service keys (1..8), listings of 4 ids (at least 1)")
    assert refusal(lambda: eng.set_receptionist(2, 0)) == (EINVAL, "the receptionist: 2 service keys (1..8), listings of 0 ids (at least 1)")
    assert refusal(lambda: eng.register_services(0, 4, 0)) == (
        EINVAL, "agx_register_services needs an engine with the receptionist (agx_set_receptionist)")
    assert refusal(eng.run) == (
        EINVAL, "agx_register_services was called on an engine without the receptionist (agx_set_receptionist)")
    eng.set_receptionist(2, 4)
    assert refusal(lambda: eng.set_receptionist(2, 4)) == (EINVAL, "the receptionist is already set (2 service keys)")
    assert refusal(lambda: eng.register_services(0, 4, 2)) == (EINVAL, "service key 2 of 2")
    assert refusal(lambda: eng.register_services(60, 5, 0)) == (EINVAL, "bad actor range")
    assert refusal(lambda: eng.read_listing(2)) == (EINVAL, "service key 2 of 2")
    eng.close()


OTHERS = {
    "priority": (lambda e: e.set_mailbox_priority(1, bytes(range(256))), "priority tables (agx_set_mailbox_priority)", "priority mailboxes need"),
    "stash": (lambda e: e.set_stash(1, 4), "a deque-based mailbox class (agx_set_stash)", "deque-based mailboxes need"),
    "timers": (lambda e: e.set_timers(1), "timers (agx_set_timers)", "timers need"),
    "watch": (lambda e: e.set_death_watch(1), "death watch (agx_set_death_watch)", "death watch needs"),
    "supervision": (lambda e: e.set_supervision([[typed.AgxSupervisor(class_mask=1, strategy=typed.SUP_RESTART, max_restarts=-1, within=1)]]),
                    "supervision (agx_set_supervision)", "supervision needs"),
}


@pytest.mark.parametrize("name", sorted(OTHERS))
def test_refuses_and_is_refused_by_another_feature(built, name):
    setter, named, needs = OTHERS[name]
    eng = plain_engine()
    setter(eng)
    assert refusal(lambda: eng.set_receptionist(1, 8)) == (EINVAL, f"the receptionist needs an engine without {named}")
    eng.close()
    eng = plain_engine()
    eng.set_receptionist(1, 8)
    assert refusal(lambda: setter(eng)) == (EINVAL, f"{needs} an engine without the receptionist (agx_set_receptionist)")
    eng.close()


def test_common_refusals(built, monkeypatch):
    eng = GpuEngine(EngineConfig(n_actors=64, n_ranks=2, rank=0))
    assert refusal(lambda: eng.set_receptionist(1, 8)) == (
        EINVAL, "the receptionist needs a single-rank engine (n_ranks is 2; the limit is 1)")
    eng.close()
    eng = GpuEngine(EngineConfig(n_actors=64, bucket_actors=32, throughput=3, capacity=0, n_words=8, max_emit=1))
    eng.register_range(0, 64, Kind.GCOUNTER)
    assert refusal(lambda: eng.set_receptionist(1, 8)) == (
        EINVAL, "the receptionist needs an engine without CRDT kinds (one is registered)")
    eng.close()
    eng = GpuEngine(EngineConfig(n_actors=64, bucket_actors=32, throughput=3, capacity=0, n_words=8, max_emit=1))
    eng.set_receptionist(1, 8)
    assert refusal(lambda: eng.register_range(0, 64, Kind.GCOUNTER)) == (
        EINVAL, "CRDT kinds cannot be registered on an engine with the receptionist (agx_set_receptionist)")
    eng.close()
    eng = plain_engine(max_emit=2)
    assert refusal(lambda: eng.set_receptionist(1, 8)) == (
        EINVAL, "the receptionist needs max_emit = 1 (it is 2): the drain for more evaluates a case more than once, and a "
                "route must take effect once")
    eng.close()
    eng = plain_engine()
    eng.tell(0, 1)
    assert eng.run().delivered == 1
    assert refusal(lambda: eng.set_receptionist(1, 8)) == (ESTATE, "set the receptionist before the first agx_run")
    eng.close()
    monkeypatch.setenv("AGX_RADIX_BITS", "3")
    monkeypatch.setenv("AGX_NO_FUSED", "1")
    monkeypatch.setenv("AGX_RING_APPLY", "1")
    from tests.prio_cases import echo_population
    eng = engine_for(echo_population(3, 8))   # bounded FIFO actors: the per-actor rings come up at the first run
    eng.tell(np.arange(8, dtype=np.uint32), 1 << 24)
    eng.run()
    assert refusal(lambda: eng.set_receptionist(1, 8)) == (
        EINVAL, "this engine keeps queued messages in bounded-mailbox rings of 8 slots, which know no receptionist: set the "
                "receptionist before the first run")
    eng.close()


def test_tables_refused_at_run(built):
    w = rc.node_workload(3)
    tb = w.behaviors
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))  # receptionist tables, no receptionist
    eng.register_range(0, 64, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    assert refusal(eng.run) == (EINVAL, "the compiled behaviours register, deregister, route, forward or read a listing, but the "
                                        "engine has no receptionist (agx_set_receptionist)")
    eng.close()
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))  # key 1 used, one key set
    eng.register_range(0, 64, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.set_receptionist(1, 8)
    assert refusal(eng.run) == (EINVAL, "the compiled behaviours use service key 1, but the receptionist has 1 keys "
                                        "(agx_set_receptionist)")
    eng.close()
    # a forward alone needs the receptionist too
    node = (typed.ReceiveBuilder.create(typed.State("a")).on_any_message(lambda m, s: [typed.self_ref(1).forward(m.payload), B.same])
            .build("f"))
    tf = typed.compile_behaviors([node])
    eng = GpuEngine(EngineConfig(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1))
    eng.register_range(0, 64, tf.kind_of(node))
    eng.set_behaviors(tf)
    assert refusal(eng.run)[0] == EINVAL
    eng.close()


def _foreign_tables(which):
    st = typed.State("a", "b")
    if which == "stash":
        return typed.Behaviors.with_stash(4, lambda buf: typed.ReceiveBuilder.create(st).on_any_message(
            lambda m, s: [s.a.inc(), buf.stash(), B.same]).build("s")), "the compiled behaviours stash or unstash_all, but no mailbox class of this engine has a stash capacity (agx_set_stash): without one every stash would overflow"
    if which == "timers":
        return typed.Behaviors.with_timers(lambda ts: typed.ReceiveBuilder.create(st).on_any_message(
            lambda m, s: [ts.start_single_timer("k", 1, 2), B.same]).build("t")), "the compiled behaviours use timers (key 0), but the engine has none (agx_set_timers; it has 0 slots)"
    if which == "watch":
        return typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [ctx.watch(typed.self_ref(1)), B.same]).build("w"), \
            "the compiled behaviours watch, unwatch or hold a signal case, but the engine has no death watch (agx_set_death_watch)"
    if which == "children":
        child = typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [B.same]).build("c")
        return typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [ctx.spawn(child), B.same]).build("p"), \
            "the compiled behaviours spawn, stop a child or read the spawn count, but the engine has no children (agx_set_children)"
    exc = typed.ExceptionType("Boom")
    return typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [s.a.inc(), B.throw(exc)]).build("x"), \
        "the compiled behaviours fail (AGX_RES_FAIL) or hold a PreRestart / PostStop signal case, but the engine has no supervision (agx_set_supervision)"


@pytest.mark.parametrize("which", ["stash", "timers", "watch", "children", "supervision"])
def test_foreign_tables_refused_on_this_engine(built, which):
    beh, text = _foreign_tables(which)
    tb = typed.compile_behaviors([beh], max_emit=1)
    eng = GpuEngine(EngineConfig(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1))
    eng.register_range(0, 64, tb.kind_of(beh))
    eng.set_behaviors(tb)
    eng.set_receptionist(1, 8)
    got = refusal(eng.run)
    eng.close()
    assert got == (EINVAL, text)
