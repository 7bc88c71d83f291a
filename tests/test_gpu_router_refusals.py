"""Every refusal of consistent-hashing and random routing (agx_set_router_logics), by status and full
text."""
import pytest

from akka_amd import typed
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 6
B = typed.Behaviors
ctx = typed.context
KEY_A, KEY_B = typed.ServiceKey("a"), typed.ServiceKey("b")
NO_RECEPTIONIST = ("router logics need an engine with the receptionist (agx_set_receptionist): a router routes through a "
                   "service key")
NO_LOGICS = ("the compiled behaviours route by consistent hashing or at random, but the engine has no router logics "
             "(agx_set_router_logics)")


def status_and_text(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]   # ("AGX_EINVAL: <the engine's text>")


def engine(n=80, **cfg):
    return GpuEngine(EngineConfig(**dict(dict(n_actors=n, throughput=4, bucket_actors=32), **cfg)))


def routing_tables(hashed=(KEY_A,), random=()):
    """one behaviour: the message k routes 7 through the k-th key, the hashed ones first"""
    st = typed.State("count", "other")
    rb = typed.ReceiveBuilder.create(st)
    for k, key in enumerate(hashed):
        rb.on_message_equals(k, (lambda key: lambda m, s: [ctx.route_hashed(key, m.arg, 7), B.same])(key))
    for k, key in enumerate(random):
        rb.on_message_equals(len(hashed) + k, (lambda key: lambda m, s: [ctx.route_random(key, 7, counter=s.count), B.same])(key))
    tb = typed.compile_behaviors([rb.on_any_message(lambda m, s: [B.same]).build("router")], max_emit=1)
    assert [a.op for a in tb.acts[:tb.n_acts]] == [typed.A_ROUTE] * (len(hashed) + len(random))
    return tb


def test_without_the_receptionist(built):
    eng = engine()
    assert status_and_text(lambda: eng.set_router_logics(1, 4, 0)) == (EINVAL, NO_RECEPTIONIST)
    assert status_and_text(lambda: eng.read_hash_ring(0)) == \
        (EINVAL, "agx_read_hash_ring needs an engine with router logics (agx_set_router_logics)")
    assert eng.router_info() == dict(hashed=0, random=0, ring_rebuilds=0, ring_size=[0] * 8)
    eng.set_receptionist(2, 80)
    assert status_and_text(lambda: eng.read_hash_ring(0)) == \
        (EINVAL, "agx_read_hash_ring needs an engine with router logics (agx_set_router_logics)")
    eng.set_router_logics(1, 4, 0)
    assert status_and_text(lambda: eng.read_hash_ring(1)) == (EINVAL, "service key 1 is not a hashed key (hashed_keys_mask 0x1)")
    assert status_and_text(lambda: eng.read_hash_ring(8)) == (EINVAL, "service key 8 is not a hashed key (hashed_keys_mask 0x1)")
    hs, ids = eng.read_hash_ring(0)
    assert len(hs) == 0 and len(ids) == 0
    eng.close()


def test_topics_in_either_order(built):
    eng = engine()
    eng.set_receptionist(1, 80)
    eng.set_topics(4)
    assert status_and_text(lambda: eng.set_router_logics(1, 4, 0)) == \
        (EINVAL, "router logics need an engine without topics (agx_set_topics): the hashed and random routes know no topics")
    eng.close()
    eng = engine()
    eng.set_receptionist(1, 80)
    eng.set_router_logics(0)
    assert status_and_text(lambda: eng.set_topics(4)) == \
        (EINVAL, "topics need an engine without router logics (agx_set_router_logics): the hashed and random routes know no "
                 "topics")
    eng.close()


def test_argument_checks(built):
    eng = engine()
    eng.set_receptionist(2, 80)
    assert status_and_text(lambda: eng.set_router_logics(4, 4, 0)) == \
        (EINVAL, "router logics: hashed_keys_mask 0x4 names a service key past the receptionist's 2")
    assert status_and_text(lambda: eng.set_router_logics(0x103, 4, 0)) == \
        (EINVAL, "router logics: hashed_keys_mask 0x103 names a service key past the receptionist's 2")
    assert status_and_text(lambda: eng.set_router_logics(1, 0, 0)) == (EINVAL, "router logics: a virtual_nodes_factor of 0 (1..64)")
    assert status_and_text(lambda: eng.set_router_logics(3, 65, 0)) == (EINVAL, "router logics: a virtual_nodes_factor of 65 (1..64)")
    eng.set_router_logics(0, 65, 0)  # (an empty mask: the factor is ignored)
    assert eng.router_info()["ring_size"] == [0] * 8
    eng.close()


def test_too_many_ring_points(built):
    eng = engine(n=(1 << 18) + 1, bucket_actors=2048)
    eng.set_receptionist(1, 8)
    assert status_and_text(lambda: eng.set_router_logics(1, 64, 0)) == \
        (EINVAL, "router logics: 262145 actors x a virtual_nodes_factor of 64 are more than 16777216 ring points")
    eng.close()


def test_once_and_before_the_first_run(built):
    eng = engine()
    eng.set_receptionist(2, 80)
    eng.set_router_logics(2, 3, 0)
    assert status_and_text(lambda: eng.set_router_logics(2, 3, 0)) == (EINVAL, "router logics are already set (hashed_keys_mask 0x2)")
    eng.close()
    eng = engine()
    eng.register_range(0, 80, 1)
    eng.set_receptionist(1, 8)
    eng.run(1)
    assert status_and_text(lambda: eng.set_router_logics(1, 3, 0)) == (ESTATE, "set router logics before the first agx_run")
    eng.close()


def test_inherits_the_receptionist_refusals(built):
    eng = engine(max_emit=2)  # (the receptionist needs max_emit = 1: no receptionist, so no router logics)
    assert status_and_text(lambda: eng.set_receptionist(1, 8))[0] == EINVAL
    assert status_and_text(lambda: eng.set_router_logics(1, 4, 0)) == (EINVAL, NO_RECEPTIONIST)
    eng.close()
    eng = engine()
    eng.set_receptionist(1, 8)
    eng.set_router_logics(1, 4, 0)
    assert status_and_text(lambda: eng.set_timers(1)) == \
        (EINVAL, "timers need an engine without the receptionist (agx_set_receptionist)")
    eng.close()


@pytest.mark.parametrize("logic", ["hashed", "random"])
def test_tables_that_use_a_logic_on_an_engine_without_the_call(built, logic):
    tb = routing_tables((KEY_A,), ()) if logic == "hashed" else routing_tables((), (KEY_A,))
    assert tb.uses_router_logics and tb.uses_receptionist
    eng = engine()
    eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.tell([3], [0])
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "the compiled behaviours register, deregister, route, forward or read a listing, but the engine has no "
                 "receptionist (agx_set_receptionist)")
    eng.set_receptionist(1, 80)
    assert status_and_text(lambda: eng.run(1)) == (EINVAL, NO_LOGICS)
    eng.set_router_logics(tb.hashed_keys_mask, 3, 1)  # (then it runs: nobody is registered)
    st = eng.run()
    assert eng.receptionist_info()["no_routees"] == 1 and st.in_flight == 0 and st.dead_letters == 1
    eng.close()


def test_a_hashed_route_through_a_key_outside_the_mask(built):
    tb = routing_tables((KEY_A, KEY_B), ())
    assert tb.hashed_keys_mask == 3
    eng = engine()
    eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.set_receptionist(2, 80)
    eng.set_router_logics(1, 3, 0)
    eng.tell([3], [1])
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "the compiled behaviours route by consistent hashing through service key 1, which is not a hashed key "
                 "(agx_set_router_logics: hashed_keys_mask 0x1)")
    eng.close()


@pytest.mark.parametrize("flags", [typed.ROUTE_HASHED | typed.ROUTE_RANDOM, typed.ROUTE_HASHED | typed.ROUTE_BY_INDEX,
                                   typed.ROUTE_RANDOM | typed.ROUTE_BY_INDEX | typed.ROUTE_KEEP_SENDER, 14])
def test_two_selection_flags_on_one_action(built, flags):
    tb = routing_tables((KEY_A, KEY_B), ())
    tb.acts[1].pad0 = flags  # the hand-made table
    eng = engine()
    eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.set_receptionist(2, 80)
    eng.set_router_logics(3, 3, 0)
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "compiled behaviours: route action 1 sets more than one of AGX_ROUTE_BY_INDEX, AGX_ROUTE_HASHED and "
                 "AGX_ROUTE_RANDOM")
    eng.close()


def test_route_flags_past_the_last(built):
    tb = routing_tables()
    eng = engine()
    tb.acts[0].pad0 = 16
    assert status_and_text(lambda: eng.set_behaviors(tb)) == \
        (EINVAL, "compiled behaviours: bad action 0 (service keys 0..7, route flags 0..15)")
    tb.acts[0].pad0 = typed.ROUTE_HASHED
    tb.acts[0].dsrc = 200  # (a hashed route reads its d-operand)
    assert status_and_text(lambda: eng.set_behaviors(tb)) == \
        (EINVAL, "compiled behaviours: bad action 0 (service keys 0..7, route flags 0..15)")
    eng.close()
