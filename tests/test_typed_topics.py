"""The DSL of pub-sub topics (akka_amd/typed.py): the lowering of every form, field by field, the
numbering of topics together with ServiceKeys, and every CompileError."""
import pytest

from akka_amd import typed
from akka_amd import workloads as wl

B = typed.Behaviors
ctx = typed.context
NEWS, SPORT = typed.Topic("news"), typed.Topic("sport")
KEY = typed.ServiceKey("news")  # (a ServiceKey and a Topic of one name are two keys)
NOTE = typed.MessageType("Note", 5)


def lower(*handlers, **kw):
    rb = typed.ReceiveBuilder.create(typed.State("cursor", "n"))
    for h in handlers:
        rb.on_any_message(h)
    b = rb.build("b")
    return typed.compile_behaviors([b], **kw), b


def test_subscribe_and_unsubscribe_lower_to_register_and_deregister():
    t, _ = lower(lambda m, s: [ctx.subscribe(NEWS), ctx.unsubscribe(SPORT), ctx.subscribe(SPORT), B.same])
    assert [(x.op, x.pad0, x.pad1, x.word, x.or_mask) for x in t.acts[:t.n_acts]] == [
        (typed.A_REGISTER, 0, 0, 0, 0), (typed.A_DEREGISTER, 0, 1, 0, 0), (typed.A_REGISTER, 0, 1, 0, 0)]
    assert t.service_keys == [NEWS, SPORT] and t.uses_receptionist and t.uses_topics and t.max_tells == 0


def test_publish_fields():
    t, _ = lower(lambda m, s: [ctx.publish(SPORT, NOTE(m.arg + 2)), B.same], lambda m, s: [ctx.publish(NEWS, s.n), B.same])
    a, b = t.acts[:2]
    assert (a.op, a.word, a.pad0, a.pad1) == (typed.A_PUBLISH, 0, 0, 0) and typed.A_PUBLISH == 22
    assert (a.src, a.k, a.or_mask) == (typed.V_ARG, 2, 5 << 24)
    assert (a.dsrc, a.dword, a.dk) == (typed.V_CONST, 0, 0)  # no destination
    assert (b.op, b.pad1, b.src, b.sword, b.or_mask) == (typed.A_PUBLISH, 1, typed.V_WORD, 1, 0)
    assert t.max_tells == 0 and t.uses_topics and t.uses_receptionist and not t.uses_forward


def test_subscriber_count_is_the_listing_size():
    rb = typed.ReceiveBuilder.create(typed.State("cursor", "n"))
    rb.on_any_message(lambda m, s: [s.n.set(ctx.subscriber_count(SPORT) + 4), B.same], when=lambda m, s: ctx.subscriber_count(NEWS) > 2)
    t = typed.compile_behaviors([rb.build("b")])
    assert t.service_keys == [NEWS, SPORT]
    c = t.cases[0]
    assert (c.src1, c.word1, c.cmp1, c.k2) == (typed.V_LISTING_SIZE, 0, typed.CMP_GT, 2)
    assert (t.acts[0].src, t.acts[0].sword, t.acts[0].k) == (typed.V_LISTING_SIZE, 1, 4)
    assert t.uses_topics


def test_topics_share_the_key_space_with_service_keys():
    t, _ = lower(lambda m, s: [ctx.register(KEY), ctx.subscribe(NEWS), ctx.publish(typed.Topic("news"), 1), ctx.deregister(KEY), B.same])
    assert t.service_keys == [KEY, NEWS] and [x.pad1 for x in t.acts[:4]] == [0, 1, 1, 0]
    keys = [typed.ServiceKey(f"k{i}") for i in range(5)]
    topics = [typed.Topic(f"t{i}") for i in range(3)]
    t, _ = lower(lambda m, s: [ctx.register(k) for k in keys] + [ctx.subscribe(x) for x in topics] + [B.same])
    assert len(t.service_keys) == 8
    with pytest.raises(typed.CompileError, match="more than 8 service keys"):
        lower(lambda m, s: [ctx.register(k) for k in keys] + [ctx.subscribe(x) for x in topics] + [ctx.subscribe(NEWS), B.same])
    t, _ = lower(lambda m, s: [ctx.register(KEY), B.same])
    assert not t.uses_topics  # (a ServiceKey alone is the receptionist's)


def test_not_a_topic():
    for call in (lambda: ctx.subscribe(KEY), lambda: ctx.unsubscribe("news"), lambda: ctx.publish(KEY, 1),
                 lambda: ctx.subscriber_count(3)):
        with pytest.raises(typed.CompileError, match="not a Topic"):
            call()
    with pytest.raises(typed.CompileError, match="not a ServiceKey"):
        ctx.register(NEWS)


def test_a_case_holds_one_of_tell_route_and_publish():
    with pytest.raises(typed.CompileError, match="a case holds 2 of tell, route and publish"):
        lower(lambda m, s: [ctx.publish(NEWS, 1), typed.self_ref(1).tell(2), B.same])
    with pytest.raises(typed.CompileError, match="a case holds 2 of tell, route and publish"):
        lower(lambda m, s: [ctx.route(KEY, 1, cursor=s.cursor), ctx.publish(NEWS, 1), B.same])
    with pytest.raises(typed.CompileError, match="a case holds 2 of tell, route and publish"):
        lower(lambda m, s: [ctx.publish(NEWS, 1), ctx.publish(SPORT, 1), B.same])
    lower(lambda m, s: [ctx.subscribe(NEWS), ctx.publish(NEWS, 1), s.n.inc(), B.same])  # (one envelope: fine)


def test_topics_live_on_the_receptionists_engine():
    with pytest.raises(typed.CompileError, match="the receptionist needs max_emit = 1"):
        lower(lambda m, s: [ctx.publish(NEWS, 1), B.same], max_emit=2)

    def with_timers(timers):
        timers.cancel("k")
        return typed.ReceiveBuilder.create(typed.State("a", "b")).on_any_message(lambda m, s: [ctx.publish(NEWS, 1), B.same]).build("b")
    with pytest.raises(typed.CompileError, match="the receptionist shares an engine with neither"):
        typed.compile_behaviors([B.with_timers(with_timers)])


def test_the_workloads_lower():
    w = wl.topic_broadcast(2, 64, 2, period=2, ticks=4)
    assert w.behaviors.uses_topics and len(w.behaviors.service_keys) == 2 and w.topics == {"log_capacity": 1024}
    assert [len(d) for d, _, _ in w.schedule] == [2, 0, 2, 0]
    assert w.receptionist["starts"] == [(2, 32, 0), (34, 32, 1)]
    w = wl.topic_mesh(256, 4, seed=3, ticks=5)
    assert w.behaviors.uses_topics and len(w.behaviors.service_keys) == 4 and len(w.schedule) == 5
    assert all(isinstance(k, typed.Topic) for k in w.behaviors.service_keys)
    assert wl.service_mesh(256, 2, 1, 2).topics == {}  # (a workload without topics: the targets are unaffected)
