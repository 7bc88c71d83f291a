"""The DSL of consistent-hashing and random routing (akka_amd/typed.py): the lowering of both
context calls and both builders, field by field, what Tables reports, and every CompileError."""
import pytest

from akka_amd import typed
from akka_amd import workloads as wl

B = typed.Behaviors
ctx = typed.context
W, V = typed.ServiceKey("worker"), typed.ServiceKey("verifier")
JOB = typed.MessageType("Job", 5)
LST = typed.MessageType("Listing", 9)


def lower(*handlers, **kw):
    rb = typed.ReceiveBuilder.create(typed.State("cursor", "n"))
    for h in handlers:
        rb.on_any_message(h)
    b = rb.build("b")
    return typed.compile_behaviors([b], **kw), b


def test_route_hashed_fields():
    assert (typed.ROUTE_HASHED, typed.ROUTE_RANDOM) == (4, 8)
    t, _ = lower(lambda m, s: [ctx.route_hashed(W, m.arg, JOB(m.arg + 1)), B.same],
                 lambda m, s: [ctx.route_hashed(V, s.n + 3, m.payload, forward=False, virtual_nodes_factor=7), B.same])
    a, b = t.acts[:2]
    assert (a.op, a.pad0, a.pad1, a.word) == (typed.A_ROUTE, typed.ROUTE_HASHED | typed.ROUTE_KEEP_SENDER, 0, 0)
    assert (a.dsrc, a.dword, a.dk) == (typed.V_ARG, 0, 0) and (a.src, a.k, a.or_mask) == (typed.V_ARG, 1, 5 << 24)
    assert (b.op, b.pad0, b.pad1) == (typed.A_ROUTE, typed.ROUTE_HASHED, 1)
    assert (b.dsrc, b.dword, b.dk) == (typed.V_WORD, 1, 3) and (b.src, b.or_mask) == (typed.V_PAYLOAD, 0)
    assert t.service_keys == [W, V] and t.hashed_keys == [0, 1] and t.hashed_keys_mask == 3
    assert t.virtual_nodes_factor == 7 and t.uses_router_logics and t.uses_receptionist and t.max_tells == 1
    assert not t.uses_topics and not t.uses_listings


def test_route_random_fields():
    t, _ = lower(lambda m, s: [ctx.route_random(W, JOB(2), counter=s.n), B.same],
                 lambda m, s: [ctx.route_random(W, m.payload, counter=s.cursor, forward=False), B.same])
    a, b = t.acts[:2]
    assert (a.op, a.pad0, a.pad1, a.word) == (typed.A_ROUTE, typed.ROUTE_RANDOM | typed.ROUTE_KEEP_SENDER, 0, 1)
    assert (a.dsrc, a.dword, a.dk) == (typed.V_CONST, 0, 0) and (a.src, a.k, a.or_mask) == (typed.V_CONST, 2, 5 << 24)
    assert (b.op, b.pad0, b.word) == (typed.A_ROUTE, typed.ROUTE_RANDOM, 0)
    assert t.hashed_keys == [] and t.hashed_keys_mask == 0 and t.virtual_nodes_factor == 0 and t.uses_router_logics


def test_the_other_logics_use_no_router_logics():
    t, _ = lower(lambda m, s: [ctx.route(W, m.payload, cursor=s.cursor), B.same],
                 lambda m, s: [ctx.route_by(W, m.arg, m.payload), B.same])
    assert not t.uses_router_logics and t.hashed_keys == [] and t.virtual_nodes_factor == 0


def test_the_builders():
    h = typed.Routers.group(W).with_consistent_hash_routing(13, lambda m: m.arg).build("hr")
    r = typed.Routers.group(V).with_random_routing().build("rr")
    rr = typed.Routers.group(V).with_round_robin_routing().build("plain")
    t = typed.compile_behaviors([h, r, rr], max_emit=1)
    acts = t.acts[:t.n_acts]
    assert [a.op for a in acts] == [typed.A_ADD, typed.A_ROUTE] * 3
    fwd = typed.ROUTE_KEEP_SENDER
    assert (acts[1].pad0, acts[1].pad1, acts[1].dsrc, acts[1].src) == (typed.ROUTE_HASHED | fwd, 0, typed.V_ARG, typed.V_PAYLOAD)
    assert (acts[3].pad0, acts[3].pad1, acts[3].word) == (typed.ROUTE_RANDOM | fwd, 1, 0)  # the counter: state word 0
    assert (acts[5].pad0, acts[5].pad1) == (fwd, 1)
    assert acts[0].word == acts[2].word == 1  # `routed` counts in state word 1
    assert t.hashed_keys == [0] and t.hashed_keys_mask == 1 and t.virtual_nodes_factor == 13 and t.uses_router_logics
    # a builder goes back to another logic
    back = typed.Routers.group(W).with_consistent_hash_routing(2, lambda m: m.arg).with_round_robin_routing().build("b")
    assert not typed.compile_behaviors([back]).uses_router_logics


def test_one_factor_per_tables():
    a = typed.Routers.group(W).with_consistent_hash_routing(3, lambda m: m.arg).build("a")
    b = typed.Routers.group(V).with_consistent_hash_routing(3, lambda m: m.arg).build("b")
    c = typed.Routers.group(V).with_consistent_hash_routing(4, lambda m: m.arg).build("c")
    assert typed.compile_behaviors([a, b]).virtual_nodes_factor == 3
    with pytest.raises(typed.CompileError, match="two hashed routers with the virtualNodesFactors 3 and 4: an engine has one"):
        typed.compile_behaviors([a, c])
    # a context call that names none takes the routers'
    t, _ = lower(lambda m, s: [ctx.route_hashed(W, m.arg, m.payload), B.same])
    assert t.virtual_nodes_factor == 0 and t.hashed_keys == [0]


@pytest.mark.parametrize("factor", [0, -1, True, 2.5])
def test_a_factor_has_to_be_a_positive_integer(factor):
    with pytest.raises(typed.CompileError) as e:
        typed.Routers.group(W).with_consistent_hash_routing(factor, lambda m: m.arg)
    assert str(e.value) == "virtualNodesFactor has to be a positive integer"


def test_a_factor_past_the_limit():
    with pytest.raises(typed.CompileError, match="virtualNodesFactor is at most 64, not 65"):
        ctx.route_hashed(W, 1, 2, virtual_nodes_factor=65)
    with pytest.raises(typed.CompileError, match="virtualNodesFactor has to be a positive integer"):
        ctx.route_hashed(W, 1, 2, virtual_nodes_factor=-3)


def test_not_with_topics_or_listings():
    news = typed.Topic("news")
    text = "hashed and random routes share an engine with neither topics nor listings"
    with pytest.raises(typed.CompileError, match=text):
        lower(lambda m, s: [ctx.route_hashed(W, m.arg, m.payload), B.same], lambda m, s: [ctx.subscribe(news), B.same])
    with pytest.raises(typed.CompileError, match=text):
        lower(lambda m, s: [ctx.route_random(W, m.payload, counter=s.n), B.same], lambda m, s: [ctx.publish(news, 1), B.same])
    with pytest.raises(typed.CompileError, match=text):
        lower(lambda m, s: [ctx.route_hashed(W, m.arg, m.payload), ctx.receptionist_find(V, LST), B.same])


def test_the_counter_is_a_state_field():
    with pytest.raises(typed.CompileError, match="counter= names a state field of the router, not 3"):
        ctx.route_random(W, 1, counter=3)
    with pytest.raises(typed.CompileError, match="counter= names a state field of the router"):
        lower(lambda m, s: [ctx.route_random(W, 1, counter=m.arg), B.same])
    with pytest.raises(typed.CompileError, match="not a ServiceKey"):
        ctx.route_hashed("worker", 1, 2)
    with pytest.raises(typed.CompileError, match="not a ServiceKey"):
        typed.Routers.group("worker")


def test_one_envelope_per_case():
    with pytest.raises(typed.CompileError, match="a case holds 2 of tell and route"):
        lower(lambda m, s: [ctx.route_hashed(W, m.arg, 1), ctx.route_random(W, 2, counter=s.n), B.same], max_emit=1)


def test_the_workloads_lower():
    w = wl.sticky_sessions(n_clients=32, n_routers=2, n_workers=8, n_spare=2, virtual_nodes_factor=5, ticks=3, join_at=1)
    tb = w.behaviors
    assert tb.uses_router_logics and tb.hashed_keys == [0] and tb.virtual_nodes_factor == 5
    assert w.router_logics == {"hashed_keys_mask": 1, "virtual_nodes_factor": 5, "seed": 1}
    assert w.receptionist["starts"] == [(34, 6, 0)] and len(w.schedule) == 3 and len(w.schedule[1][0]) == 34
    w = wl.random_pool(n_routers=4, n_workers=8, ticks=2)
    assert w.behaviors.uses_router_logics and w.router_logics["hashed_keys_mask"] == 0
