"""The DSL of the receptionist and the group routers (akka_amd/typed.py): the lowering, field by
field, every CompileError, and the numbering of the service keys."""
import pytest

from akka_amd import typed
from akka_amd import workloads as wl

B = typed.Behaviors
ctx = typed.context
K0, K1 = typed.ServiceKey("jobs"), typed.ServiceKey("logs")
JOB = typed.MessageType("Job", 5)


def lower(*handlers, state=None, **kw):
    rb = typed.ReceiveBuilder.create(state or typed.State("cursor", "n"))
    for h in handlers:
        rb.on_any_message(h)
    b = rb.build("b")
    return typed.compile_behaviors([b], **kw), b


def test_register_and_deregister_lower_to_the_key_in_pad1():
    t, _ = lower(lambda m, s: [ctx.register(K0), ctx.deregister(K1), ctx.register(K1), B.same])
    a = t.acts[:t.n_acts]
    assert [(x.op, x.pad0, x.pad1, x.word, x.or_mask) for x in a] == [
        (typed.A_REGISTER, 0, 0, 0, 0), (typed.A_DEREGISTER, 0, 1, 0, 0), (typed.A_REGISTER, 0, 1, 0, 0)]
    assert t.service_keys == [K0, K1] and t.uses_receptionist and not t.uses_forward and t.max_tells == 0


def test_route_round_robin_fields():
    t, _ = lower(lambda m, s: [ctx.route(K0, JOB(m.arg + 2), cursor=s.n), B.same])
    a = t.acts[0]
    assert (a.op, a.word, a.pad0, a.pad1) == (typed.A_ROUTE, 1, typed.ROUTE_KEEP_SENDER, 0)
    assert (a.src, a.k, a.or_mask) == (typed.V_ARG, 2, 5 << 24)
    assert t.max_tells == 1 and t.uses_forward


def test_route_without_forward_and_route_by_fields():
    t, _ = lower(lambda m, s: [ctx.route(K0, m.payload, cursor=s.cursor, forward=False), B.same],
                 lambda m, s: [ctx.route_by(K1, m.arg + 3, m.payload), B.same],
                 lambda m, s: [ctx.route_by(K1, s.n, 7, forward=False), B.same])
    a, b, c = t.acts[:3]
    assert (a.op, a.word, a.pad0, a.pad1, a.src) == (typed.A_ROUTE, 0, 0, 0, typed.V_PAYLOAD)
    assert (b.op, b.pad0, b.pad1, b.dsrc, b.dk) == (typed.A_ROUTE, typed.ROUTE_BY_INDEX | typed.ROUTE_KEEP_SENDER, 1, typed.V_ARG, 3)
    assert (c.pad0, c.dsrc, c.dword, c.src, c.k) == (typed.ROUTE_BY_INDEX, typed.V_WORD, 1, typed.V_CONST, 7)


def test_ref_forward_sets_the_flag_on_a_tell():
    t, _ = lower(lambda m, s: [typed.self_ref(1).forward(JOB(m.arg)), B.same], lambda m, s: [typed.self_ref(1).tell(1), B.same])
    assert [(x.op, x.pad0) for x in t.acts[:2]] == [(typed.A_TELL, typed.ROUTE_KEEP_SENDER), (typed.A_TELL, 0)]
    assert t.uses_forward and t.uses_receptionist and t.service_keys == []


def test_listing_size_and_service_at_operands():
    rb = typed.ReceiveBuilder.create(typed.State("cursor", "n"))
    rb.on_any_message(lambda m, s: [s.n.set(ctx.listing_size(K1) + 4), ctx.service_at(K1, s.n + 1).tell(1),
                                    B.same], when=lambda m, s: ctx.listing_size(K0) > 2)
    rb.on_any_message(lambda m, s: [ctx.service_at(K0, m.arg).tell(2), B.same])
    rb.on_any_message(lambda m, s: [ctx.service_at(K0, 9).tell(3), B.same])
    t = typed.compile_behaviors([rb.build("b")])
    assert t.service_keys == [K0, K1]  # the test of the first case names K0 first
    c = t.cases[0]
    assert (c.src1, c.word1, c.k1, c.cmp1, c.src2, c.k2) == (typed.V_LISTING_SIZE, 0, 0, typed.CMP_GT, typed.V_CONST, 2)
    a = t.acts[:4]
    assert (a[0].src, a[0].sword, a[0].k) == (typed.V_LISTING_SIZE, 1, 4)
    assert (a[1].dsrc, a[1].dword, a[1].dk) == (typed.V_SERVICE_AT, 1 | (typed.SVC_WORD1 << 3), 1)
    assert (a[2].dsrc, a[2].dword, a[2].dk) == (typed.V_SERVICE_AT, 0 | (typed.SVC_ARG << 3), 0)
    assert (a[3].dsrc, a[3].dword, a[3].dk) == (typed.V_SERVICE_AT, 0 | (typed.SVC_CONST << 3), 9)


def test_keys_are_numbered_in_order_of_first_appearance_and_by_name():
    k = [typed.ServiceKey(f"k{i}") for i in range(8)]
    t, _ = lower(lambda m, s: [ctx.register(k[3]), ctx.register(typed.ServiceKey("k1")), ctx.register(k[3]), ctx.register(k[0]), B.same])
    assert t.service_keys == [k[3], k[1], k[0]]
    assert [x.pad1 for x in t.acts[:4]] == [0, 1, 0, 2]
    t, _ = lower(lambda m, s: [ctx.register(x) for x in k] + [B.same])
    assert len(t.service_keys) == 8


def test_group_router_builders():
    r = typed.Routers.group(K0).build("r")
    assert r.state.names == ("cursor", "routed")
    t = typed.compile_behaviors([r], max_emit=1)
    a = t.acts[:t.n_acts]
    assert [(x.op, x.word) for x in a] == [(typed.A_ADD, 1), (typed.A_ROUTE, 0)]
    assert (a[1].pad0, a[1].src) == (typed.ROUTE_KEEP_SENDER, typed.V_PAYLOAD)
    r2 = typed.Routers.group(K0).with_round_robin_routing().with_index_routing(lambda m: m.arg).build("r2")
    a = typed.compile_behaviors([r2]).acts[1]
    assert (a.op, a.pad0, a.dsrc) == (typed.A_ROUTE, typed.ROUTE_BY_INDEX | typed.ROUTE_KEEP_SENDER, typed.V_ARG)


def test_compile_errors():
    with pytest.raises(typed.CompileError, match="more than 8 service keys"):
        lower(lambda m, s: [ctx.register(typed.ServiceKey(f"k{i}")) for i in range(9)] + [B.same])
    with pytest.raises(typed.CompileError, match="not a ServiceKey"):
        ctx.register("jobs")
    with pytest.raises(typed.CompileError, match="cursor= names a state field"):
        ctx.route(K0, 1, cursor=3)
    with pytest.raises(typed.CompileError, match="service_at takes"):
        ctx.service_at(K0, typed.Incoming.payload)
    with pytest.raises(typed.CompileError, match="needs max_emit = 1, not 2"):
        lower(lambda m, s: [ctx.register(K0), B.same], max_emit=2)
    with pytest.raises(typed.CompileError, match="holds 2 of tell and route"):
        lower(lambda m, s: [ctx.route(K0, 1, cursor=s.cursor), m.sender.tell(1), B.same])
    with pytest.raises(typed.CompileError, match="holds 2 of tell and route"):
        lower(lambda m, s: [typed.self_ref(1).forward(1), m.sender.tell(1), B.same])


def _with(which):
    st = typed.State("cursor", "n")
    reg = ctx.register(K0)
    if which == "stash":
        return B.with_stash(4, lambda buf: typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [reg, buf.stash(), B.same]).build("s"))
    if which == "timers":
        return B.with_timers(lambda ts: typed.ReceiveBuilder.create(st).on_any_message(
            lambda m, s: [reg, ts.start_single_timer("k", 1, 2), B.same]).build("t"))
    if which == "watch":
        return typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [reg, ctx.watch(m.sender), B.same]).build("w")
    if which == "children":
        child = typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [B.same]).build("c")
        return typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [reg, ctx.spawn(child), B.same]).build("p")
    if which == "receive_timeout":
        return typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [reg, ctx.set_receive_timeout(3, 1), B.same]).build("r")
    return typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [reg, B.throw(typed.ExceptionType("Boom"))]).build("x")


@pytest.mark.parametrize("which", ["stash", "timers", "watch", "children", "receive_timeout", "supervision"])
def test_no_other_feature_beside_the_receptionist(which):
    with pytest.raises(typed.CompileError, match="the receptionist shares an engine with neither"):
        typed.compile_behaviors([_with(which)])


def test_tables_without_the_receptionist_are_unchanged():
    t = typed.compile_behaviors(list(typed.library().values()))
    assert not t.uses_receptionist and not t.uses_forward and t.service_keys == []
    assert all(a.pad0 == 0 and a.pad1 == 0 for a in t.acts[:t.n_acts])


def test_workloads_carry_the_receptionist():
    w = wl.service_pool(4, 16, ticks=3)
    assert w.receptionist == {"n_keys": 1, "capacity": 16, "starts": [(4, 16, 0)]} and w.behaviors.uses_receptionist
    assert len(w.schedule) == 3 and w.max_emit == 1
    w = wl.service_mesh(256, n_keys=8, ticks=5)
    assert w.receptionist["n_keys"] == 8 == len(w.behaviors.service_keys) and len(w.schedule) == 5
    calls = []

    class T:
        def __getattr__(self, name):
            return lambda *a, **k: calls.append(name)
    w.apply_to(T())
    assert calls.index("set_behaviors") < calls.index("set_receptionist") < calls.index("register_services")
