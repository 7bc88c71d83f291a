"""The lowering of context.receptionist_subscribe / receptionist_find: action codes, pad1, the Listing
payloads, and every CompileError."""
import pytest

from akka_amd import typed
from tests import listing_cases as lc

B = typed.Behaviors
ctx = typed.context
KEY_A, KEY_B = typed.ServiceKey("a"), typed.ServiceKey("b")
LISTING_A, LISTING_B = typed.MessageType("ListingA", 9), typed.MessageType("ListingB", 10)


def build(*handlers):
    st = typed.State("count", "other")
    rb = typed.ReceiveBuilder.create(st)
    for k, h in enumerate(handlers):
        rb.on_message_equals(k, h)
    return typed.compile_behaviors([rb.on_any_message(lambda m, s: [B.same]).build("b")], max_emit=1)


def test_action_codes():
    assert (typed.A_SUBSCRIBE_LISTING, typed.A_FIND) == (23, 24)


def test_lowering():
    tb = build(lambda m, s: [ctx.receptionist_subscribe(KEY_B, LISTING_B), B.same],
               lambda m, s: [ctx.receptionist_find(KEY_A, LISTING_A), s.count.inc(), B.same])
    a = tb.acts
    assert (a[0].op, a[0].pad1, a[0].pad0) == (typed.A_SUBSCRIBE_LISTING, 0, 0)  # (KEY_B appears first: key 0)
    assert (a[1].op, a[1].pad1, a[1].pad0) == (typed.A_FIND, 1, 0) and a[2].op == typed.A_ADD
    assert tb.service_keys == [KEY_B, KEY_A] and tb.listing_types == {0: LISTING_B, 1: LISTING_A}
    assert tb.listing_payloads == [(10 << 24) | 0, (9 << 24) | 1]
    assert tb.uses_listings and tb.uses_receptionist and not tb.uses_topics and tb.max_tells == 0


def test_neither_is_an_envelope_of_the_case():
    tb = build(lambda m, s: [ctx.receptionist_subscribe(KEY_A, LISTING_A), ctx.receptionist_find(KEY_B, LISTING_B),
                             typed.self_ref(1).tell(3), B.same],
               lambda m, s: [ctx.receptionist_find(KEY_A, LISTING_A), ctx.route(KEY_A, 5, cursor=s.other), B.same],
               lambda m, s: [ctx.receptionist_subscribe(KEY_A, LISTING_A), ctx.publish(typed.Topic("t"), 5), B.same])
    assert tb.max_tells == 1 and tb.uses_topics and tb.uses_listings
    assert tb.listing_payloads == [LISTING_A.payload(0), LISTING_B.payload(1), 0]  # (nobody asks for the topic's listing)


def test_a_key_without_a_listing_has_payload_zero():
    tb = build(lambda m, s: [ctx.register(KEY_A), B.same], lambda m, s: [ctx.receptionist_find(KEY_B, LISTING_B), B.same])
    assert tb.listing_payloads == [0, LISTING_B.payload(1)]
    assert not build(lambda m, s: [ctx.register(KEY_A), B.same]).uses_listings


def test_handlers_are_ordinary_cases():
    st = typed.State("size", "first")
    beh = (typed.ReceiveBuilder.create(st)
           .on_message(LISTING_A, lambda m, s: [s.size.set(ctx.listing_size(KEY_A)), s.first.set(ctx.service_at(KEY_A, 0).dst), B.same])
           .on_any_message(lambda m, s: [ctx.receptionist_subscribe(KEY_A, LISTING_A), B.same]).build("w"))
    tb = typed.compile_behaviors([beh], max_emit=1)
    assert tb.acts[0].src == typed.V_LISTING_SIZE and tb.acts[1].src == typed.V_SERVICE_AT and tb.acts[2].op == typed.A_SUBSCRIBE_LISTING


def test_one_message_type_per_key():
    with pytest.raises(typed.CompileError, match="one message type per key"):
        build(lambda m, s: [ctx.receptionist_subscribe(KEY_A, LISTING_A), B.same],
              lambda m, s: [ctx.receptionist_find(KEY_A, LISTING_B), B.same])
    # the same type again, and one type for two keys (the argument tells them apart), are fine
    tb = build(lambda m, s: [ctx.receptionist_subscribe(KEY_A, LISTING_A), B.same],
               lambda m, s: [ctx.receptionist_find(KEY_A, LISTING_A), B.same],
               lambda m, s: [ctx.receptionist_find(KEY_B, LISTING_A), B.same])
    assert tb.listing_payloads == [LISTING_A.payload(0), LISTING_A.payload(1)]


@pytest.mark.parametrize("act", [ctx.receptionist_subscribe, ctx.receptionist_find])
def test_compile_errors(act):
    with pytest.raises(typed.CompileError, match="a Topic has no Listing"):
        act(typed.Topic("news"), LISTING_A)
    with pytest.raises(typed.CompileError, match="not a ServiceKey"):
        act("a", LISTING_A)
    with pytest.raises(typed.CompileError, match="the Listing of a key is a MessageType"):
        act(KEY_A, 9)
    with pytest.raises(typed.CompileError, match="the Listing of a key is a MessageType"):
        act(KEY_A, LISTING_A(0))


def test_more_than_eight_keys():
    hs = [(lambda k: lambda m, s: [ctx.receptionist_find(typed.ServiceKey(f"k{k}"), LISTING_A), B.same])(k) for k in range(9)]
    with pytest.raises(typed.CompileError, match="more than 8 service keys"):
        build(*hs)


def test_the_scenario_tables():
    node, tb = lc.node_tables(64)
    assert tb.listing_payloads == [lc.LISTING[0].payload(0), lc.LISTING[1].payload(1), 0] and tb.uses_listings and tb.uses_topics
