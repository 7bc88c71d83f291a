"""The children surface of the compiled-behaviour DSL (akka_amd.typed: context.spawn / stop / child_at / spawned),
without a GPU: the lowering of each call and every CompileError."""
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.typed import CompileError

B = typed.Behaviors
ctx = typed.context
ST = typed.State("a", "b")


def lower(*behaviors, max_emit=1):
    return typed.compile_behaviors(list(behaviors), max_emit=max_emit)


def leaf(name="leaf"):
    return typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [s.a.inc(), B.same]).build(name)


def test_spawn_encoding_and_sites():
    """dword is the site, the operand the argument, pad0 & 1 the receiving word; equal sites are shared; a spawned
    behaviour is a reachable root"""
    kid, other = leaf("kid"), leaf("other")
    b = (typed.ReceiveBuilder.create(ST)
         .on_any_message(lambda m, s: [ctx.spawn(kid, arg=m.arg, word1=ctx.PARENT, into=s.b), B.same], test=lambda m: m.tag == 1)
         .on_any_message(lambda m, s: [ctx.spawn(kid, arg=s.a - 1, word1=ctx.PARENT), B.same], test=lambda m: m.tag == 2)
         .on_any_message(lambda m, s: [ctx.spawn(other, arg=5, word1=77, base=1000), B.same])
         .build("p"))
    tb = lower(b)
    assert [x.name for x in tb.behaviors] == ["p", "kid", "other"]
    acts = [tb.acts[i] for i in range(3)]  # (the parent's three cases; the children's own actions follow)
    assert [a.op for a in acts] == [typed.A_SPAWN] * 3 == [13] * 3
    assert (acts[0].dword, acts[0].pad0, acts[0].word, acts[0].src) == (0, 1, 1, typed.V_ARG)
    assert (acts[1].dword, acts[1].pad0, acts[1].src, acts[1].sword, acts[1].k) == (0, 0, typed.V_WORD, 0, -1)
    assert (acts[2].dword, acts[2].pad0, acts[2].src, acts[2].k) == (1, 0, typed.V_CONST, 5)
    assert tb.spawn_sites == [(typed.KIND_COMPILED + 1, 0, None), (typed.KIND_COMPILED + 2, 1000, 77)]
    assert tb.uses_children and not tb.uses_watch and tb.max_tells == 0


def test_stop_child_at_and_spawned():
    b = (typed.ReceiveBuilder.create(ST)
         .on_any_message(lambda m, s: [ctx.stop(s.b.ref), B.same], test=lambda m: m.tag == 1)
         .on_any_message(lambda m, s: [ctx.child_at(s.a).tell(m.payload), s.a.inc(), B.same], when=lambda m, s: ctx.spawned > 0)
         .on_any_message(lambda m, s: [ctx.stop(ctx.child_at(3)), s.a.set(ctx.spawned), B.same])
         .build("p"))
    tb = lower(b)
    acts = [tb.acts[i] for i in range(tb.n_acts)]
    assert (acts[0].op, acts[0].dsrc, acts[0].dword) == (typed.A_STOP_CHILD, typed.V_WORD, 1) and typed.A_STOP_CHILD == 14
    assert (acts[1].op, acts[1].dsrc, acts[1].dword, acts[1].dk) == (typed.A_TELL, typed.V_CHILD, 0, 0)
    assert (acts[3].dsrc, acts[3].dword, acts[3].dk) == (typed.V_CHILD, typed.CHILD_NO_WORD, 3)
    assert (acts[4].src, acts[4].k) == (typed.V_SPAWNED, 0) and (typed.V_SPAWNED, typed.V_CHILD) == (9, 10)
    c = tb.cases[1]
    assert (c.src1, c.cmp1, c.src2, c.k2) == (typed.V_SPAWNED, typed.CMP_GT, typed.V_CONST, 0)
    assert tb.uses_children and not tb.spawn_sites
    offs = typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [ctx.child_at(s.b + 2).tell(1), B.same]).build("o")
    a = lower(offs).acts[0]
    assert (a.dsrc, a.dword, a.dk) == (typed.V_CHILD, 1, 2)


def test_uses_children_only_from_an_operand():
    b = typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [B.same], when=lambda m, s: ctx.spawned == 0).build("o")
    assert lower(b).uses_children
    assert not lower(leaf()).uses_children


def test_workloads_lower():
    w = wl.spawn_tree(3, 2)
    assert w.behaviors.uses_children and w.children["sites"] == [(typed.KIND_COMPILED, 0, None)]
    assert w.children["regions"] == [(0, 1, 1, 2), (1, 2, 3, 2), (3, 4, 7, 2)] and w.n_actors == 15
    p = wl.pool_router(4, 16)
    assert p.behaviors.uses_children and p.behaviors.uses_watch and p.watch["n_slots"] == 4
    assert p.children["regions"] == [(0, 4, 4, 16)] and len(p.children["spawns"]) == 16


@pytest.mark.parametrize("effects", [
    lambda s, kid: [ctx.spawn(kid), typed.self_ref(1).tell(1)],
    lambda s, kid: [ctx.spawn(kid), ctx.spawn(kid)],
    lambda s, kid: [ctx.spawn(kid, into=s.a), ctx.stop(s.a.ref)],
    lambda s, kid: [ctx.stop(s.a.ref), typed.actor_ref(99).tell(1)],
])
def test_one_emitting_action_per_case(effects):
    kid = leaf()
    b = typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: effects(s, kid) + [B.same]).build("two")
    with pytest.raises(CompileError, match="tell, spawn and stop"):
        lower(b)


def test_spawn_argument_must_fit():
    kid = leaf()
    ctx.spawn(kid, arg=(1 << 18) - 1)
    for bad in (1 << 18, -1):
        with pytest.raises(CompileError, match="18 bits"):
            ctx.spawn(kid, arg=bad)


def test_bad_spawn_arguments():
    kid = leaf()
    with pytest.raises(CompileError, match="Behavior"):
        ctx.spawn("kid")
    with pytest.raises(CompileError, match="word 1"):
        ctx.spawn(kid, word1=ST.a)
    with pytest.raises(CompileError, match="word 1"):
        ctx.spawn(kid, word1=-1)
    with pytest.raises(CompileError, match="base"):
        ctx.spawn(kid, base=1 << 64)
    with pytest.raises(CompileError, match="into="):
        ctx.spawn(kid, into=3)
    with pytest.raises(CompileError, match="ActorRef"):
        ctx.stop(5)
    with pytest.raises(CompileError, match="child_at"):
        ctx.child_at(typed.Incoming.arg)


@pytest.mark.parametrize("tag", [typed.TAG_CREATE, typed.TAG_STOP])
def test_reserved_tags(tag):
    assert (typed.TAG_CREATE, typed.TAG_STOP) == (0xFD, 0xFC)
    kid = leaf()
    spawn = lambda m, s: [ctx.spawn(kid), B.same]
    sends = (typed.ReceiveBuilder.create(ST).on_any_message(spawn, test=lambda m: m.tag == 1)
             .on_any_message(lambda m, s: [typed.self_ref(1).tell(0, tag=tag), B.same]).build("sends"))
    with pytest.raises(CompileError, match="reserved for Create and Stop"):
        lower(sends)
    tests_ = (typed.ReceiveBuilder.create(ST).on_any_message(spawn, test=lambda m: m.tag == 1)
              .on_message(typed.MessageType("X", tag), lambda m, s: [B.same]).build("tests"))
    with pytest.raises(CompileError, match="reserved for Create and Stop"):
        lower(tests_)
    plain = typed.ReceiveBuilder.create(ST).on_message(typed.MessageType("X", tag), lambda m, s: [B.same]).build("plain")
    lower(plain)  # (without children the tags are ordinary ones)


def test_children_share_no_engine_with_timers_stash_or_supervision():
    spawn = lambda m, s: [ctx.spawn(leaf()), B.same]  # (a fresh child each time: with_timers marks what it reaches)
    t = B.with_timers(lambda ts: typed.ReceiveBuilder.create(ST).on_any_message(spawn, test=lambda m: m.tag == 1)
                      .on_any_message(lambda m, s: [ts.start_single_timer("k", 1, 2), B.same]).build("t"))
    with pytest.raises(CompileError, match="children"):
        lower(t)
    st = B.with_stash(4, lambda buf: typed.ReceiveBuilder.create(ST).on_any_message(spawn, test=lambda m: m.tag == 1)
                      .on_any_message(lambda m, s: [buf.stash(), B.same]).build("s"))
    with pytest.raises(CompileError, match="children"):
        lower(st)
    sv = typed.ReceiveBuilder.create(ST).on_any_message(spawn).build("sv")
    B.supervise(sv).on_failure(typed.SupervisorStrategy.restart)
    with pytest.raises(CompileError, match="children"):
        lower(sv)
    with pytest.raises(CompileError, match="max_emit"):
        lower(typed.ReceiveBuilder.create(ST).on_any_message(spawn).build("e"), max_emit=2)


def test_too_many_sites():
    kids = [leaf(f"k{i}") for i in range(3)]
    rb = typed.ReceiveBuilder.create(ST)
    for i in range(typed.MAX_SPAWN_SITES + 1):
        rb.on_any_message(lambda m, s, i=i: [ctx.spawn(kids[i % 3], base=i), B.same], test=lambda m, i=i: m.arg == i)
    with pytest.raises(CompileError, match="spawn sites"):
        lower(rb.build("many"))
