"""Every refusal of pub-sub topics (agx_set_topics), by status and full text."""
import pytest

from akka_amd import typed
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 6
B = typed.Behaviors
ctx = typed.context
NEWS, SPORT = typed.Topic("news"), typed.Topic("sport")


def status_and_text(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]   # ("AGX_EINVAL: <the engine's text>")


def engine(n=80, **cfg):
    return GpuEngine(EngineConfig(**dict(dict(n_actors=n, throughput=4, bucket_actors=32), **cfg)))


def publishing_tables(topics=(NEWS,)):
    """one behaviour: the message k publishes 7 to topic k"""
    st = typed.State("count", "other")
    rb = typed.ReceiveBuilder.create(st)
    for k, tp in enumerate(topics):
        rb.on_message_equals(k, (lambda tp: lambda m, s: [ctx.publish(tp, 7), B.same])(tp))
    tb = typed.compile_behaviors([rb.on_any_message(lambda m, s: [B.same]).build("publisher")], max_emit=1)
    assert [a.op for a in tb.acts[:tb.n_acts]] == [typed.A_PUBLISH] * len(topics)
    return tb


def test_argument_checks_and_the_receptionist_first(built):
    eng = engine()
    assert status_and_text(lambda: eng.set_topics(0)) == (EINVAL, "topics: a log of 0 publications per tick (1..65536)")
    assert status_and_text(lambda: eng.set_topics(65537)) == (EINVAL, "topics: a log of 65537 publications per tick (1..65536)")
    assert status_and_text(lambda: eng.set_topics(16)) == \
        (EINVAL, "topics need an engine with the receptionist (agx_set_receptionist): a topic is a service key")
    assert status_and_text(lambda: eng.publish(0, 1)) == (EINVAL, "agx_publish needs an engine with topics (agx_set_topics)")
    assert status_and_text(eng.read_topic_log) == (EINVAL, "agx_read_topic_log needs an engine with topics (agx_set_topics)")
    assert eng.topic_info() == dict(published=0, fanned_out=0, no_subscribers=0, host_published=0)
    eng.set_receptionist(2, 80)
    assert status_and_text(lambda: eng.publish(0, 1)) == (EINVAL, "agx_publish needs an engine with topics (agx_set_topics)")
    eng.set_topics(65536)
    assert status_and_text(lambda: eng.publish(2, 1)) == (EINVAL, "topic 2 of 2")
    eng.close()


def test_inherits_the_receptionist_refusals(built):
    eng = engine(max_emit=2)  # (the receptionist needs max_emit = 1: no receptionist, so no topics)
    assert status_and_text(lambda: eng.set_receptionist(1, 8))[0] == EINVAL
    assert status_and_text(lambda: eng.set_topics(16)) == \
        (EINVAL, "topics need an engine with the receptionist (agx_set_receptionist): a topic is a service key")
    eng.close()
    eng = engine()
    eng.set_receptionist(1, 8)
    eng.set_topics(16)
    assert status_and_text(lambda: eng.set_timers(1)) == \
        (EINVAL, "timers need an engine without the receptionist (agx_set_receptionist)")
    eng.close()


def test_once_and_before_the_first_run(built):
    eng = engine()
    eng.set_receptionist(1, 8)
    eng.set_topics(16)
    assert status_and_text(lambda: eng.set_topics(16)) == (EINVAL, "topics are already set (a log of 16 publications)")
    eng.close()
    eng = engine()
    eng.register_range(0, 80, 1)
    eng.set_receptionist(1, 8)
    eng.run(1)
    assert status_and_text(lambda: eng.set_topics(16)) == (ESTATE, "set topics before the first agx_run")
    eng.close()


def test_tables_that_publish_on_an_engine_without_topics(built):
    tb = publishing_tables()
    assert tb.uses_topics and tb.uses_receptionist and tb.service_keys == [NEWS]
    eng = engine()
    eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.tell([3], [0])
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "the compiled behaviours register, deregister, route, forward or read a listing, but the engine has no "
                 "receptionist (agx_set_receptionist)")
    eng.set_receptionist(1, 80)
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "the compiled behaviours publish, but the engine has no topics (agx_set_topics)")
    eng.set_topics(8)  # (then it runs)
    st = eng.run()
    assert eng.topic_info() == dict(published=1, fanned_out=0, no_subscribers=1, host_published=0) and st.in_flight == 0
    eng.close()


def test_a_topic_past_n_keys(built):
    tb = publishing_tables((NEWS, SPORT))
    eng = engine()
    eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.set_receptionist(1, 80)
    eng.set_topics(8)
    eng.tell([3], [1])
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "the compiled behaviours use service key 1, but the receptionist has 1 keys (agx_set_receptionist)")
    eng.close()


def test_publish_plus_tell_in_one_case(built):
    st = typed.State("count", "other")
    both = (typed.ReceiveBuilder.create(st)
            .on_any_message(lambda m, s: [s.count.inc(), typed.self_ref(1).tell(1), B.same]).build("teller"))
    tb = typed.compile_behaviors([both], max_emit=1)
    assert tb.acts[1].op == typed.A_TELL
    pub = publishing_tables()
    # the hand-made table: the case's ADD becomes a PUBLISH beside its TELL
    tb.acts[0].op, tb.acts[0].pad1, tb.acts[0].pad0 = typed.A_PUBLISH, 0, 0
    eng = engine()
    assert status_and_text(lambda: eng.set_behaviors(tb)) == \
        (EINVAL, "compiled behaviours: case 0 holds 2 of tell, route and publish; an engine with topics has max_emit 1")
    for field, value in (("pad0", 1), ("pad1", 8)):
        setattr(pub.acts[0], field, value)
        assert status_and_text(lambda: eng.set_behaviors(pub)) == \
            (EINVAL, "compiled behaviours: bad action 0 (service keys 0..7, route flags 0..3)"), field
        setattr(pub.acts[0], field, 0)
    eng.set_behaviors(pub)
    eng.close()
