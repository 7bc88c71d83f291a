"""Every refusal of Subscribe / Listing (agx_set_listings), by status and full text."""
import pytest

from akka_amd import typed
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 6
B = typed.Behaviors
ctx = typed.context
KEY_A, KEY_B = typed.ServiceKey("a"), typed.ServiceKey("b")
LISTING_A, LISTING_B = typed.MessageType("ListingA", 9), typed.MessageType("ListingB", 10)
NO_TOPICS = ("listings need an engine with topics (agx_set_topics after agx_set_receptionist): a Listing is injected as a "
             "publication's delivery is")
NO_LISTINGS = "the compiled behaviours subscribe to or find a listing, but the engine has no listings (agx_set_listings)"


def status_and_text(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]   # ("AGX_EINVAL: <the engine's text>")


def engine(n=80, **cfg):
    return GpuEngine(EngineConfig(**dict(dict(n_actors=n, throughput=4, bucket_actors=32), **cfg)))


def listing_tables(find=False, keys=((KEY_A, LISTING_A),)):
    """one behaviour: the message k subscribes to (or finds) key k"""
    st = typed.State("count", "other")
    rb = typed.ReceiveBuilder.create(st)
    act = ctx.receptionist_find if find else ctx.receptionist_subscribe
    for k, (key, msg) in enumerate(keys):
        rb.on_message_equals(k, (lambda key, msg: lambda m, s: [act(key, msg), B.same])(key, msg))
    tb = typed.compile_behaviors([rb.on_any_message(lambda m, s: [s.count.inc(), B.same]).build("subscriber")], max_emit=1)
    assert [a.op for a in tb.acts[:len(keys)]] == [typed.A_FIND if find else typed.A_SUBSCRIBE_LISTING] * len(keys)
    return tb


def test_without_topics_in_either_order(built):
    eng = engine()
    assert status_and_text(lambda: eng.set_listings([1 << 24])) == (EINVAL, NO_TOPICS)
    eng.set_receptionist(1, 80)
    assert status_and_text(lambda: eng.set_listings([1 << 24])) == (EINVAL, NO_TOPICS)
    eng.set_topics(1)  # (a log of one publication is enough for someone who publishes nothing)
    eng.set_listings([1 << 24])
    eng.close()


def test_the_calls_on_an_engine_without_listings(built):
    eng = engine()
    eng.set_receptionist(1, 80)
    eng.set_topics(1)
    assert status_and_text(lambda: eng.subscribe_listings(0, 4, 0)) == \
        (EINVAL, "agx_subscribe_listings needs an engine with listings (agx_set_listings)")
    assert status_and_text(eng.listing_info) == (EINVAL, "agx_listing_info needs an engine with listings (agx_set_listings)")
    assert status_and_text(eng.read_subscriptions) == \
        (EINVAL, "agx_read_subscriptions needs an engine with listings (agx_set_listings)")
    eng.close()


def test_twice_the_key_count_and_the_arguments(built):
    eng = engine()
    eng.set_receptionist(2, 80)
    eng.set_topics(4)
    assert status_and_text(lambda: eng.set_listings([1 << 24])) == \
        (EINVAL, "listings: 1 Listing payloads, but the receptionist has 2 keys (agx_set_receptionist)")
    assert status_and_text(lambda: eng.set_listings([1 << 24] * 3)) == \
        (EINVAL, "listings: 3 Listing payloads, but the receptionist has 2 keys (agx_set_receptionist)")
    eng.set_listings([1 << 24, 2 << 24])
    assert status_and_text(lambda: eng.set_listings([1 << 24, 2 << 24])) == (EINVAL, "listings are already set (2 keys)")
    assert status_and_text(lambda: eng.subscribe_listings(0, 4, 2)) == (EINVAL, "service key 2 of 2")
    assert status_and_text(lambda: eng.subscribe_listings(78, 4, 0)) == (EINVAL, "actors [78, 82) of 80")
    assert status_and_text(lambda: eng.read_subscriptions(78, 4)) == (EINVAL, "actors [78, 82) of 80")
    assert eng.listing_info() == dict(subscribes=0, finds=0, listings_sent=0, notified=0)
    eng.close()


def test_after_the_first_run(built):
    eng = engine()
    eng.register_range(0, 80, 1)
    eng.set_receptionist(1, 8)
    eng.set_topics(4)
    eng.run(1)
    assert status_and_text(lambda: eng.set_listings([1 << 24])) == (ESTATE, "set listings before the first agx_run")
    eng.close()


def test_inherits_the_receptionist_refusals(built):
    eng = engine(max_emit=2)  # (the receptionist needs max_emit = 1: no receptionist, no topics, so no listings)
    assert status_and_text(lambda: eng.set_receptionist(1, 8))[0] == EINVAL
    assert status_and_text(lambda: eng.set_listings([1 << 24])) == (EINVAL, NO_TOPICS)
    eng.close()
    eng = engine()
    eng.set_receptionist(1, 8)
    eng.set_topics(4)
    eng.set_listings([1 << 24])
    assert status_and_text(lambda: eng.set_timers(1)) == \
        (EINVAL, "timers need an engine without the receptionist (agx_set_receptionist)")
    eng.close()


@pytest.mark.parametrize("find", [False, True])
def test_tables_with_the_actions_on_an_engine_without_listings(built, find):
    tb = listing_tables(find)
    assert tb.uses_listings and tb.uses_receptionist and not tb.uses_topics and tb.listing_payloads == [LISTING_A.payload(0)]
    eng = engine()
    eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.tell([3], [0])
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "the compiled behaviours register, deregister, route, forward or read a listing, but the engine has no "
                 "receptionist (agx_set_receptionist)")
    eng.set_receptionist(1, 80)
    assert status_and_text(lambda: eng.run(1)) == (EINVAL, NO_LISTINGS)
    eng.set_topics(1)
    assert status_and_text(lambda: eng.run(1)) == (EINVAL, NO_LISTINGS)
    eng.set_listings(tb.listing_payloads)  # (then it runs: the Listing is the behaviour's second message)
    st = eng.run()
    assert st.delivered == 2 and st.in_flight == 0
    assert eng.listing_info() == dict(subscribes=0 if find else 1, finds=1 if find else 0, listings_sent=1, notified=0)
    sub, pend = eng.read_subscriptions(3, 1)
    assert (int(sub[0]), int(pend[0])) == (0 if find else 1, 0) and eng.read_state()[0][3].tolist() == [1, 0]
    eng.close()


def test_a_key_past_n_keys(built):
    tb = listing_tables(keys=((KEY_A, LISTING_A), (KEY_B, LISTING_B)))
    eng = engine()
    eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.set_receptionist(1, 80)
    eng.set_topics(1)
    eng.set_listings([LISTING_A.payload(0)])
    eng.tell([3], [1])
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "the compiled behaviours use service key 1, but the receptionist has 1 keys (agx_set_receptionist)")
    eng.close()


def test_bad_action_fields(built):
    tb = listing_tables()
    eng = engine()
    for field, value in (("pad0", 1), ("pad1", 8)):
        setattr(tb.acts[0], field, value)
        assert status_and_text(lambda: eng.set_behaviors(tb)) == \
            (EINVAL, "compiled behaviours: bad action 0 (service keys 0..7, route flags 0..3)"), field
        setattr(tb.acts[0], field, 0)
    eng.set_behaviors(tb)
    eng.close()
