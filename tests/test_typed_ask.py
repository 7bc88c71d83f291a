"""context.ask in the typed DSL (akka_amd/typed.py): the lowering to AGX_A_ASK_ARM + AGX_A_ASK_SEND
with exact agx_act fields, the timer keys it takes, and every CompileError."""
import pytest

from akka_amd import typed
from akka_amd.typed import (A_ASK_ARM, A_ASK_SEND, A_TELL, A_TIMER_PERIODIC, CMP_EQ, V_ARG, V_CONST, V_SELF, V_TIMER,
                            V_WORD, CompileError)

B = typed.Behaviors
ctx = typed.context
REQ, ANS, TMO, TICK = (typed.MessageType(n, t) for n, t in (("Req", 2), ("Ans", 4), ("Tmo", 5), ("Tick", 1)))


def fields(a):
    return dict(op=a.op, word=a.word, src=a.src, sword=a.sword, k=a.k, dsrc=a.dsrc, dword=a.dword, dk=a.dk,
                or_mask=a.or_mask, pad0=a.pad0, pad1=a.pad1)


def client(handler, setup=None, extra=()):
    st = typed.State("count", "server")

    def build(timers):
        if setup:
            setup(timers)
        rb = typed.ReceiveBuilder.create(st).on_message(TICK, lambda m, s: handler(m, s, timers))
        for mt, h in extra:
            rb.on_message(mt, h)
        return rb.on_any_message(lambda m, s: [B.unhandled]).build("client")
    return B.with_timers(build)


def test_lowering_exact_fields():
    b = client(lambda m, s, t: [ctx.ask(s.server.ref, REQ(m.arg), 4, on_timeout=TMO(9), on_success=ANS), B.same],
               setup=lambda t: t.start_timer_with_fixed_delay("tick", TICK(), 8))
    tb = typed.compile_behaviors([b], max_emit=1)
    assert tb.uses_ask and tb.timer_keys == 2 and tb.max_tells == 1 and not tb.uses_receive_timeout
    assert tb.initial_timers == [(typed.KIND_COMPILED, 0, True, 8, 1 << 24)]
    c = tb.cases[0]
    assert (c.act_first, c.act_count) == (0, 2)
    assert fields(tb.acts[0]) == dict(op=A_ASK_ARM, word=1, src=V_CONST, sword=0, k=9, dsrc=V_CONST, dword=0, dk=4,
                                      or_mask=5 << 24, pad0=1, pad1=4)
    assert fields(tb.acts[1]) == dict(op=A_ASK_SEND, word=1, src=V_ARG, sword=0, k=0, dsrc=V_WORD, dword=1, dk=0,
                                      or_mask=2 << 24, pad0=0, pad1=0)
    assert tb.n_acts == 2


def test_no_mapping_a_computed_timeout_and_a_self_based_target():
    b = client(lambda m, s, t: [s.count.inc(), ctx.ask(typed.self_ref(3), 7, s.count + 1, on_timeout=0x05000000), B.same])
    tb = typed.compile_behaviors([b], max_emit=1)
    assert tb.timer_keys == 1 and [a.op for a in tb.acts[:tb.n_acts]] == [typed.A_ADD, A_ASK_ARM, A_ASK_SEND]
    assert fields(tb.acts[1]) == dict(op=A_ASK_ARM, word=0, src=V_CONST, sword=0, k=0x05000000, dsrc=V_WORD, dword=0, dk=1,
                                      or_mask=0, pad0=0, pad1=0)
    assert fields(tb.acts[2]) == dict(op=A_ASK_SEND, word=0, src=V_CONST, sword=0, k=7, dsrc=V_SELF, dword=0, dk=3,
                                      or_mask=0, pad0=0, pad1=0)


def test_each_ask_site_takes_a_key_in_order_of_appearance_with_the_timers():
    b = client(lambda m, s, t: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO()), B.same],
               setup=lambda t: t.cancel("first"),
               extra=[(ANS, lambda m, s: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO()), B.same]),
                      (TMO, lambda m, s: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO(), key="shared"), B.same]),
                      (REQ, lambda m, s: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO(), key="shared"), B.same])])
    tb = typed.compile_behaviors([b], max_emit=1)
    assert [a.word for a in tb.acts[:tb.n_acts] if a.op == A_ASK_ARM] == [1, 2, 3, 3] and tb.timer_keys == 4


def test_ask_pending_is_the_timer_operand_of_the_key():
    st = typed.State("count", "server")

    def build(timers):
        return (typed.ReceiveBuilder.create(st)
                .on_message(TICK, lambda m, s: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO(), key="a"), B.same],
                            when=lambda m, s: ctx.ask_pending("a"))
                .on_any_message(lambda m, s: [B.unhandled]).build("c"))
    tb = typed.compile_behaviors([B.with_timers(build)], max_emit=1)
    c = tb.cases[0]
    assert (c.src3, c.word3, c.cmp2, c.src4, c.k4) == (V_TIMER, 0, CMP_EQ, V_CONST, 1)


# ------------------------------------------------------------------ every CompileError, each with its own text
def err(build, **kw):
    with pytest.raises(CompileError) as e:
        typed.compile_behaviors([build() if callable(build) else build], **kw)
    return str(e.value)


def test_outside_with_timers():
    with pytest.raises(CompileError, match="context.ask lives inside Behaviors.with_timers"):
        ctx.ask(typed.actor_ref(1), REQ(), 2, on_timeout=TMO())
    with pytest.raises(CompileError, match="context.ask lives inside Behaviors.with_timers"):
        ctx.ask_pending("a")


def test_a_fifth_key():
    def build():
        return client(lambda m, s, t: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO()), B.same],
                      setup=lambda t: [t.cancel(k) for k in "abcd"])
    assert "an ask takes a timer key and an actor has at most 4: this ask would be key 5" in err(build)


def test_a_constant_timeout_below_one():
    def build():
        return client(lambda m, s, t: [ctx.ask(s.server.ref, REQ(), 0, on_timeout=TMO()), B.same])
    assert err(build) == "an ask's timeout is at least 1 tick, not 0"


def test_on_success_takes_a_message_type():
    def build():
        return client(lambda m, s, t: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO(), on_success=4), B.same])
    assert err(build) == "on_success= takes a MessageType or None, not 4"


def test_a_tell_or_a_second_ask_in_the_case():
    def tell():
        return client(lambda m, s, t: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO()), typed.self_ref(1).tell(REQ()), B.same])

    def two():
        return client(lambda m, s, t: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO()),
                                       ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO()), B.same])
    for build in (tell, two):
        assert err(build, max_emit=1) == ("a case holds 2 of tell and ask: an ask's request is the case's one envelope, and "
                                          "an engine with ask has max_emit 1")


def test_max_emit_above_one():
    def build():
        return client(lambda m, s, t: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO()), B.same])
    assert err(build, max_emit=2) == "ask needs max_emit = 1, not 2"


SHARES = ("ask lives on the timer engine, which shares an engine with neither a stash, death watch, children, supervision, "
          "the receptionist nor receive timeouts: the behaviours ask and use one of them")


def asking(extra):
    return client(lambda m, s, t: [ctx.ask(s.server.ref, REQ(), 2, on_timeout=TMO()), B.same], extra=extra)


def test_together_with_another_feature():
    key = typed.ServiceKey("svc")
    child = typed.ReceiveBuilder.create(typed.State("a", "b")).on_any_message(lambda m, s: [B.same]).build("child")
    others = {
        "watch": [(ANS, lambda m, s: [ctx.watch(s.server.ref), B.same])],
        "children": [(ANS, lambda m, s: [ctx.spawn(child), B.same])],
        "receptionist": [(ANS, lambda m, s: [ctx.register(key), B.same])],
        "receive timeouts": [(ANS, lambda m, s: [ctx.set_receive_timeout(3, TMO()), B.same])],
        "supervision": [(ANS, lambda m, s: [B.throw(typed.ExceptionType("Boom"))])],
    }
    for name, extra in others.items():
        assert err(lambda: asking(extra), max_emit=1) == SHARES, name

    def stash():
        def build(buf):
            return asking([(ANS, lambda m, s: [buf.stash(), B.same])])
        return B.with_stash(4, build)
    assert err(stash, max_emit=1) == SHARES
