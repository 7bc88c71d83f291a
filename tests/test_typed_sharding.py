"""The DSL of sharded entities (akka_amd/typed.py: EntityTypeKey, Entity, context.passivate): the
lowering and every CompileError.  No GPU."""
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from tests import sharding_cases as sc

B = typed.Behaviors
ctx = typed.context
JOB, IDLE, BYE = (typed.MessageType(n, t) for n, t in (("Job", 1), ("Idle", 2), ("Bye", 3)))
KEY = typed.EntityTypeKey("counter")


def entity(extra=None, state=None):
    st = state or typed.State("jobs", "id")
    rb = (typed.ReceiveBuilder.create(st)
          .on_message(JOB, lambda m, s: [s.jobs.inc(), B.same])
          .on_message(IDLE, extra or (lambda m, s: [ctx.passivate(), B.same]))
          .on_message(BYE, lambda m, s: [B.stopped]))
    return rb.build("entity")


def declared(beh, **kw):
    return typed.Entity(KEY, beh, 8, 24, **kw).with_stop_message(BYE())


def raises(text, fn):
    with pytest.raises(typed.CompileError) as e:
        fn()
    assert text in str(e.value), str(e.value)


# ------------------------------------------------------------------ the lowering
def test_passivate_lowers_to_one_action_without_operands():
    beh = entity()
    tb = typed.compile_behaviors([], max_emit=1, entities=[declared(beh)])
    a = [tb.acts[i] for i in range(tb.n_acts) if tb.acts[i].op == typed.A_PASSIVATE]
    assert typed.A_PASSIVATE == 25 and len(a) == 1
    assert (a[0].word, a[0].src, a[0].k, a[0].dsrc, a[0].dk, a[0].or_mask, a[0].pad0, a[0].pad1) == (0, typed.V_CONST, 0, typed.V_CONST, 0, 0, 0, 0)
    assert tb.uses_sharding and not tb.uses_receive_timeout and tb.timer_keys == 0 and tb.max_tells == 0


def test_entity_types_row():
    beh = entity()
    ent = typed.Entity(KEY, beh, 8, 24, word0=5, word1=typed.Entity.ID).with_stop_message(BYE(7)).with_receive_timeout(4, IDLE())
    other = typed.Entity(typed.EntityTypeKey("other"), beh, 40, 2, word1=9).with_stop_message(0x03000000)
    tb = typed.compile_behaviors([], max_emit=1, entities=[ent, other])
    k = tb.kind_of(beh)
    assert tb.entity_types == [(8, 24, k, 5, None, BYE.payload(7), 4, IDLE.payload()), (40, 2, k, 0, 9, 0x03000000, 0, 0)]
    assert k == typed.KIND_COMPILED and tb.n_behaviors == 1   # (one behaviour, lowered once)


def test_entity_behaviours_are_lowered_with_the_roots():
    beh = entity()
    plain = typed.ReceiveBuilder.create(typed.State("n", "u")).on_any_message(lambda m, s: [s.n.inc(), B.same]).build("plain")
    tb = typed.compile_behaviors([plain], max_emit=1, entities=[declared(beh)])
    assert tb.kind_of(plain) == typed.KIND_COMPILED and tb.kind_of(beh) == typed.KIND_COMPILED + 1
    assert tb.entity_types[0][2] == typed.KIND_COMPILED + 1
    tb = typed.compile_behaviors([beh, plain], max_emit=1, entities=[declared(beh)])   # (a root already: not twice)
    assert tb.n_behaviors == 2 and tb.entity_types[0][2] == typed.KIND_COMPILED


def test_passivate_without_a_declaration_still_needs_the_engine():
    tb = typed.compile_behaviors([entity()], max_emit=1)
    assert tb.uses_sharding and tb.entity_types == []


def test_refs_to_entities_are_ordinary_ids():
    st = typed.State("jobs", "peer")
    beh = entity(lambda m, s: [s.peer.ref.tell(JOB()), B.same], st)
    fwd = typed.ReceiveBuilder.create(typed.State("n", "u")).on_any_message(lambda m, s: [m.sender.tell(JOB()), B.same]).build("f")
    tb = typed.compile_behaviors([fwd], max_emit=1, entities=[declared(beh, word1=12)])
    assert tb.entity_types[0][4] == 12 and tb.uses_sharding


def test_the_workloads_declare_their_entities():
    for w in (wl.sharded_entities(96, idle=3, ticks=4, bucket_actors=32), wl.passivation_race(96, bucket_actors=32)):
        tb = w.behaviors
        assert tb.uses_sharding and tb.entity_types == [(8, 96, tb.entity_types[0][2], 0, None, wl.SE_BYE << 24, tb.entity_types[0][6], wl.SE_IDLE << 24)]
        assert w.timers["receive_timeout"]["sharding"] == tb.entity_types and w.timers["n_keys"] == 1
        assert all(first + count <= 8 for first, count, *_ in w.ranges)   # (no entity id is registered)
    w = sc.kat_workload(3)
    assert [t[:2] for t in w.behaviors.entity_types] == [sc.COUNTER, sc.IDLE]


# ------------------------------------------------------------------ the CompileErrors
def test_passivate_beside_a_tell():
    beh = entity(lambda m, s: [typed.actor_ref(3).tell(JOB()), ctx.passivate(), B.same])
    raises("a case holds 2 of tell, spawn, ask and passivate", lambda: typed.compile_behaviors([], max_emit=1, entities=[declared(beh)]))


def test_passivate_beside_a_spawn():
    child = typed.ReceiveBuilder.create(typed.State("a", "b")).on_any_message(lambda m, s: [B.same]).build("child")
    beh = entity(lambda m, s: [ctx.spawn(child), ctx.passivate(), B.same])
    raises("a case holds 2 of tell, spawn, ask and passivate", lambda: typed.compile_behaviors([], max_emit=1, entities=[declared(beh)]))


def test_passivate_beside_an_ask():
    st = typed.State("jobs", "id")

    def build(timers):
        return (typed.ReceiveBuilder.create(st)
                .on_message(IDLE, lambda m, s: [ctx.ask(typed.actor_ref(3), JOB(), 4, BYE()), ctx.passivate(), B.same])
                .build("asker"))
    beh = B.with_timers(build)
    raises("a case holds 2 of tell, spawn, ask and passivate", lambda: typed.compile_behaviors([], max_emit=1, entities=[declared(beh)]))


def test_two_passivates_in_one_case():
    beh = entity(lambda m, s: [ctx.passivate(), ctx.passivate(), B.same])
    raises("a case holds 2 of tell, spawn, ask and passivate", lambda: typed.compile_behaviors([], max_emit=1, entities=[declared(beh)]))


def shared_engine_error(other):
    raises("sharding lives on the receive-timeout engine", lambda: typed.compile_behaviors([other], max_emit=1, entities=[declared(entity())]))


def test_with_a_stash():
    buf = typed.StashBuffer(4)
    shared_engine_error(typed.ReceiveBuilder.create(typed.State("a", "b")).on_any_message(lambda m, s: [buf.stash(), B.same]).build("stasher"))


def test_with_death_watch():
    shared_engine_error(typed.ReceiveBuilder.create(typed.State("a", "b"))
                        .on_any_message(lambda m, s: [ctx.watch(typed.actor_ref(1)), B.same]).build("watcher"))


def test_with_children():
    child = typed.ReceiveBuilder.create(typed.State("a", "b")).on_any_message(lambda m, s: [B.same]).build("child")
    shared_engine_error(typed.ReceiveBuilder.create(typed.State("a", "b"))
                        .on_any_message(lambda m, s: [ctx.spawn(child), B.same]).build("parent"))


def test_with_supervision():
    boom = typed.ExceptionType("Boom")
    worker = typed.ReceiveBuilder.create(typed.State("a", "b")).on_any_message(lambda m, s: [B.throw(boom)]).build("worker")
    shared_engine_error(B.supervise(worker).on_failure(typed.SupervisorStrategy.resume))


def test_with_ask():
    def build(timers):
        return (typed.ReceiveBuilder.create(typed.State("a", "b"))
                .on_message(JOB, lambda m, s: [ctx.ask(typed.actor_ref(3), JOB(), 4, BYE()), B.same]).build("asker"))
    shared_engine_error(B.with_timers(build))


def test_with_the_receptionist():
    key = typed.ServiceKey("workers")
    shared_engine_error(typed.ReceiveBuilder.create(typed.State("a", "b"))
                        .on_any_message(lambda m, s: [ctx.register(key), B.same]).build("worker"))


def test_max_emit():
    raises("sharding needs max_emit = 1, not 2", lambda: typed.compile_behaviors([], max_emit=2, entities=[declared(entity())]))


def test_entity_type_without_a_stop_message():
    ent = typed.Entity(KEY, entity(), 8, 24)
    raises("entity type 'counter' has no stop message", lambda: typed.compile_behaviors([], max_emit=1, entities=[ent]))


def test_bad_declarations():
    beh = entity()
    raises("Entity takes an EntityTypeKey", lambda: typed.Entity("counter", beh, 8, 24))
    raises("Entity takes a Behavior", lambda: typed.Entity(KEY, B.same, 8, 24))
    raises("an entity range is", lambda: typed.Entity(KEY, beh, 8, 0))
    raises("an entity's word 1 is a u64 constant or Entity.ID", lambda: typed.Entity(KEY, beh, 8, 24, word1=-1))
    raises("an entity's word 0 is a u64 constant", lambda: typed.Entity(KEY, beh, 8, 24, word0="x"))
    raises("an entity's receive timeout is 1..", lambda: declared(beh).with_receive_timeout(0, IDLE()))
    raises("an entity's stop message is a constant message", lambda: typed.Entity(KEY, beh, 8, 24).with_stop_message(BYE(typed.Operand(typed.V_SELF))))
    raises("entities= takes Entity declarations", lambda: typed.compile_behaviors([], max_emit=1, entities=[beh]))
    two = [declared(beh), typed.Entity(typed.EntityTypeKey("b"), beh, 31, 4).with_stop_message(BYE())]
    raises("the ranges of entity types 'counter' and 'b' overlap", lambda: typed.compile_behaviors([], max_emit=1, entities=two))
    nine = [typed.Entity(typed.EntityTypeKey(str(i)), beh, 100 + i, 1).with_stop_message(BYE()) for i in range(9)]
    raises("more than 8 entity types", lambda: typed.compile_behaviors([], max_emit=1, entities=nine))


def test_reserved_tags_in_a_declaration():
    beh = entity()
    bad = typed.Entity(KEY, beh, 8, 24).with_stop_message(typed.MessageType("T", 0xFF)())
    raises("its stop message carries a reserved tag", lambda: typed.compile_behaviors([], max_emit=1, entities=[bad]))
    bad = declared(beh).with_receive_timeout(3, typed.MessageType("R", 0xFB)())
    raises("its receive-timeout message carries a reserved tag", lambda: typed.compile_behaviors([], max_emit=1, entities=[bad]))
