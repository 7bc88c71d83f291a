"""Receive timeouts on the GPU (agx_set_receive_timeout; dungeon/ReceiveTimeout.scala:18-74): the HIP engine through
the C ABI against the known answers restated from the reference's ReceiveTimeoutSpec and ActorContextSpec
(tests/golden/receive_timeout_kats.json) and against the model of DESIGN.md §2.7 (tests/receive_timeout_model.py,
itself pinned to the timers' model and the known answers by tests/test_receive_timeout_model.py), on the fused and
the multi-pass pipelines.  Populations of 80 actors in buckets of 32 (a partial last bucket).  The observable for
order is an echo to a host id (the outbox keeps each sender's order)."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import NO_SENDER, EngineConfig, GpuEngine, Kind
from tests import receive_timeout_cases as rc
from tests.prio_model import per_sender
from tests.receive_timeout_model import ReceiveTimeoutModel

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 6
NONE = 0xFFFFFFFF
P = rc.payload
B = typed.Behaviors


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the timers' fixture; NO_FUSED: populations of one digit)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def model_for(w):
    m = ReceiveTimeoutModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def targets(w):
    return engine_for(w), model_for(w)


def tell_actor(target, *msgs, actor=rc.ACTOR):
    p = np.asarray([P(m) for m in msgs], np.uint32)
    target.tell(np.full(p.size, actor, np.uint32), p, np.full(p.size, NO_SENDER, np.uint32))


def ordered(d, s, p):
    """the outbox as [dst], [src], [payload] in canonical order: by sender, each sender's messages in its order"""
    o = per_sender(d, s, p)
    return [o[1].tolist(), o[0].tolist(), o[2].tolist()]


def snapshot(target, st):
    """everything observable: counters, both infos, every actor's timeout, state words, alive flags, the outbox"""
    st = rc.counts(st)
    ti, ri = target.timer_info(), target.receive_timeout_info()
    assert rc.conserved(st, ti, ri), (st, ti, ri)
    r = target.read_receive_timeout()
    words, alive = target.read_state()
    return dict(counts=st, timer_info=ti, info=ri, rt={k: r[k].tolist() for k in ("delay", "remaining", "payload")},
                words=words.tolist(), alive=(alive & 1).tolist(), echo=ordered(*target.take_outbound()))


def status_and_text(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]   # ("AGX_EINVAL: <the engine's text>")


# ------------------------------------------------------------------ 1. the known answers
@pytest.mark.parametrize("T", rc.KAT_T)
@pytest.mark.parametrize("name", rc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(rc.kat_workload(name, T))
    got = rc.run_kat(name, T, eng)
    eng.close()
    print(got)
    rc.check_kat(name, T, got)
    assert got == rc.run_kat(name, T, model_for(rc.kat_workload(name, T)))


# ------------------------------------------------------------------ 2. a bucket whose only work is a fire
def test_fire_only_bucket(built, pipeline):
    """one timeout of 7 ticks in the partial last bucket, no mail at all; its handler turns it off"""
    eng = engine_for(rc.target_workload("off", 7, 3))
    eng.start_receive_timeout(70, 1, 7, P("Timeout"))
    ticks, echoes, again = [], [], []
    for budget in (3, 3, None):
        st = eng.run() if budget is None else eng.run(budget)
        ticks.append(eng.timer_info()["ticks"])
        echoes.append(eng.take_outbound()[2].tolist())
        again.append(eng.pump_idle())  # (a pending receive timeout keeps the pump scheduled)
    info, tinfo = eng.receive_timeout_info(), eng.timer_info()
    eng.close()
    assert ticks == [3, 6, 7] and echoes == [[], [], [P("GotTimeout")]] and again == [True, True, False]
    assert info == dict(fired=1, discarded=0, set=0, pending=0)
    assert tinfo == dict(fired=0, discarded=0, active=0, pending=0, ticks=7)  # (agx_timer_info counts timer slots only)
    assert st.supersteps == 1 and st.delivered == 1 and st.in_flight == 0  # (only tick 7 had mail)


# ------------------------------------------------------------------ 3. the inbox order of a tick
def test_inbox_order(built, pipeline):
    """an arrival, a staged tell, two timer keys and the receive timeout due in one tick, in that order"""
    st = typed.State("count", "unused")
    host = typed.actor_ref(rc.HOST)
    made = {}

    def build(timers):
        timers.cancel(0), timers.cancel(1)  # (the keys 0 and 1)
        made["echo"] = (typed.ReceiveBuilder.create(st)
                        .on_any_message(lambda m, s: [s.count.inc(), host.tell(m.payload), B.same]).build("echo"))
        return (typed.ReceiveBuilder.create(st)
                .on_any_message(lambda m, s: [typed.self_ref(1).tell(m.payload), B.same]).build("fwd"))
    fwd = B.with_timers(build)
    echo = made["echo"]
    tb = typed.compile_behaviors([fwd, echo], max_emit=1)
    w = wl.Workload("rt_order", 80, 2, 1, 5, 0, [(0, 80, tb.kind_of(echo), None), (8, 1, tb.kind_of(fwd), None)],
                    behaviors=tb, outbound=(rc.HOST, 1), bucket_actors=32,
                    timers={"n_keys": 2, "receive_timeout": {"starts": [(9, 1, 2, 0x05000005)]}})
    got = []
    for target in targets(w):
        target.start_timers(9, 1, 1, 2, payload=0x01000001)  # key 1 first: the order is by key, not by start
        target.start_timers(9, 1, 0, 2, payload=0x01000000)
        target.tell(8, 0x03000003)          # tick 1: actor 8 forwards it: an arrival for actor 9 at tick 2
        target.run(1)
        target.tell(9, 0x04000004)          # staged for tick 2
        s = snapshot(target, target.run(1))
        got.append(s)
        target.close()
    assert got[0]["echo"][2] == [0x03000003, 0x04000004, 0x01000000, 0x01000001, 0x05000005] and got[0] == got[1]


# ------------------------------------------------------------------ 4. one drained window
@pytest.mark.parametrize("order", ["set_then_cancel", "cancel_then_set"])
def test_set_and_cancel_in_one_window(built, pipeline, order):
    """throughput 5: SetTimeout(4) and the cancelling TransparentTick drained in one window -- the last one wins, the
    next fire is written once; then a Tick in the window behind them does or does not influence"""
    msgs = ["SetTimeout:4", "TransparentTick", "Tick"] if order == "set_then_cancel" else ["TransparentTick", "SetTimeout:4", "Tick"]
    got = []
    for target in targets(rc.target_workload("tt_cancels", 5, 5, initial=[(rc.ACTOR, 1, 9, "Timeout")])):
        tell_actor(target, *msgs)
        a = snapshot(target, target.run(1))
        b = snapshot(target, target.run(6))
        got.append((a, b))
        target.close()
    assert got[0] == got[1]
    a, b = got[0]
    if order == "set_then_cancel":
        assert a["info"] == dict(fired=0, discarded=0, set=0, pending=0) and a["rt"]["remaining"][rc.ACTOR] == NONE
        assert b["timer_info"]["ticks"] == 1 and b["echo"][2] == []   # (quiescent after tick 1)
    else:
        assert a["info"] == dict(fired=0, discarded=0, set=1, pending=1) and a["rt"]["delay"][rc.ACTOR] == 4
        assert a["rt"]["remaining"][rc.ACTOR] == 4 and b["echo"][2] == [P("GotTimeout")] and b["timer_info"]["ticks"] == 7


# ------------------------------------------------------------------ 5. no generation: the stale envelope
def test_stale_envelope_carries_the_replaced_message(built, pipeline):
    """throughput 1: the envelope of tick 1 waits behind a SetTimeout whose case replaces delay and message; it is
    delivered with the message stored at receipt, and influences"""
    got = []
    for target in targets(rc.target_workload("plain", 5, 1, initial=[(rc.ACTOR, 1, 1, "Ping")])):
        tell_actor(target, "SetTimeout:50")
        got.append(snapshot(target, target.run(2)))
        target.close()
    assert got[0] == got[1]
    s = got[0]
    assert s["echo"][2] == [P("TimeoutSet"), P("GotTimeout")] and s["info"] == dict(fired=1, discarded=0, set=1, pending=1)
    assert s["rt"]["remaining"][rc.ACTOR] == 50 and s["rt"]["payload"][rc.ACTOR] == P("Timeout")


def test_envelope_discarded_after_a_cancel(built, pipeline):
    """throughput 1: the envelope of tick 1 waits behind the cancelling TransparentTick: discarded, not unhandled"""
    got = []
    for target in targets(rc.target_workload("tt_cancels", 5, 1, initial=[(rc.ACTOR, 1, 1, "Timeout")])):
        tell_actor(target, "TransparentTick")
        got.append(snapshot(target, target.run()))
        target.close()
    assert got[0] == got[1]
    s = got[0]
    assert s["info"] == dict(fired=1, discarded=1, set=0, pending=0) and s["counts"]["delivered"] == 2
    assert s["counts"]["unhandled"] == 0 and s["timer_info"]["ticks"] == 2 and s["echo"][2] == []


# ------------------------------------------------------------------ 6. what does not influence
def test_queued_mail_does_not_influence(built, pipeline):
    """throughput 1 with a backlog of Ticks: only the drained one of each tick pushes the fire"""
    got = []
    for target in targets(rc.target_workload("plain", 3, 1, initial=[(rc.ACTOR, 1, 3, "Timeout")])):
        tell_actor(target, "Tick", "Tick", "Tick", "Tick", "Tick")
        steps = [snapshot(target, target.run(1)) for _ in range(9)]
        got.append(steps)
        target.close()
    assert got[0] == got[1]
    rem = [s["rt"]["remaining"][rc.ACTOR] for s in got[0]]
    assert rem == [3, 3, 3, 3, 3, 2, 1, 3, 2]   # ticks 1..5 drain one Tick each; the fire of tick 8 reschedules itself
    assert [s["echo"][2] for s in got[0]] == [[]] * 7 + [[P("GotTimeout")], []]
    assert got[0][0]["counts"]["in_flight"] == 4


def test_bounded_mailbox_envelope_is_a_dead_letter(built, pipeline):
    """capacity 1: at tick 2 a staged Tick takes the only place, the envelope dies at admission (`fired` counts it);
    the Tick reschedules, and the envelope of tick 4 is admitted"""
    got = []
    for target in targets(rc.target_workload("plain", 2, 1, initial=[(rc.ACTOR, 1, 2, "Timeout")], capacity=1)):
        target.run(1)
        tell_actor(target, "Tick")
        a = snapshot(target, target.run(1))
        b = snapshot(target, target.run(2))
        got.append((a, b))
        target.close()
    assert got[0] == got[1]
    a, b = got[0]
    assert a["info"] == dict(fired=1, discarded=0, set=1, pending=1) and a["counts"]["dead_letters"] == 1
    assert a["rt"]["remaining"][rc.ACTOR] == 2 and a["echo"][2] == []
    assert b["info"]["fired"] == 2 and b["echo"][2] == [P("GotTimeout")] and b["counts"]["dead_letters"] == 1


def test_transparent_and_influencing_timer_messages(built, pipeline):
    """a periodic timer of 3 ticks and a timeout of 4: with a transparent message the timeout fires at tick 4, with
    an influencing one every TimerMsg pushes it and it never fires (the tag is that of the slot's stored payload)"""
    got = {}
    for msg in ("TransparentTick", "Tick"):
        w = rc.target_workload("plain", 4, 5, initial=[(rc.ACTOR, 1, 4, "Timeout")], timers=[(rc.ACTOR, 1, 3, msg)])
        pair = []
        for target in targets(w):
            pair.append(snapshot(target, target.run(10)))
            target.close()
        assert pair[0] == pair[1]
        got[msg] = pair[0]
    assert got["TransparentTick"]["echo"][2] == [P("GotTimeout"), P("GotTimeout")]     # ticks 4 and 8
    assert got["TransparentTick"]["info"]["fired"] == 2 and got["TransparentTick"]["rt"]["remaining"][rc.ACTOR] == 2
    assert got["Tick"]["echo"][2] == [] and got["Tick"]["info"]["fired"] == 0
    assert got["Tick"]["rt"]["remaining"][rc.ACTOR] == 3   # (the TimerMsg of tick 9 pushed it to 13)


# ------------------------------------------------------------------ 7. stop and become
def test_stop_turns_it_off_and_become_keeps_it(built, pipeline):
    got = []
    for target in targets(rc.become_workload(3, 4)):
        target.start_receive_timeout(50, 1, 4, P("Timeout"))
        tell_actor(target, "Become")
        tell_actor(target, "Stop", actor=50)
        a = snapshot(target, target.run(5))   # tick 1: the become and the stop; tick 5: the become's actor fires
        tell_actor(target, "Stop")
        b = snapshot(target, target.run())
        got.append((a, b))
        target.close()
    assert got[0] == got[1]
    a, b = got[0]
    assert a["echo"][2] == [P("GotTimeoutB")] and a["info"] == dict(fired=1, discarded=0, set=1, pending=1)
    assert a["alive"][50] == 0 and a["rt"]["delay"][50] == 0 and a["rt"]["remaining"][50] == NONE
    assert b["info"] == dict(fired=1, discarded=0, set=0, pending=0) and b["timer_info"]["ticks"] == 6


# ------------------------------------------------------------------ 8. a random script against the model
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_script(built, pipeline, seed):
    """40 ticks of sets, cancels, transparent and plain tells and stops over three handler variants"""
    rng = np.random.default_rng(seed)
    ranges = [(0, 30, "plain"), (30, 25, "tt_cancels"), (55, 25, "tt_sets")]
    w = rc.target_workload(["plain", "tt_cancels", "tt_sets"], 3, 2, initial=[(10, 40, 4, "Timeout")], ranges=ranges,
                           timers=[(12, 1, 3, "TransparentTick"), (33, 2, 2, "Tick")])
    menu = ["SetTimeout:1", "SetTimeout:2", "SetTimeout:5", "TransparentTick", "TransparentTick", "Identify", "Tick", "Tick",
            "Ping", "Stop", "Schedule"]
    script = []
    for _ in range(40):
        k = int(rng.integers(0, 12))
        dst = rng.integers(0, rc.N_KAT + 2, k).astype(np.uint32)   # (ids 80, 81: unknown refs, dead letters)
        pay = np.asarray([P(menu[int(i)]) for i in rng.integers(0, len(menu), k)], np.uint32)
        script.append((dst, pay))
    eng, mod = targets(w)
    for t, (dst, pay) in enumerate(script):
        for target in (eng, mod):
            if dst.size:
                target.tell(dst, pay, np.full(dst.size, NO_SENDER, np.uint32))
        g, m = snapshot(eng, eng.run(1)), snapshot(mod, mod.run(1))
        assert g == m, (seed, t, {k: (g[k], m[k]) for k in g if g[k] != m[k]})
    seen = g["info"]
    eng.close()
    assert seen["fired"] > 20 and seen["discarded"] > 0 and 0 < seen["set"] and sum(g["alive"]) < rc.N_KAT


# ------------------------------------------------------------------ 9. the passivating entities
def test_passivating_entities(built, pipeline):
    w = wl.passivating_entities(96, 3, idle=3)
    eng, mod = targets(w)
    g, m = snapshot(eng, w.run_schedule(eng)), snapshot(mod, w.run_schedule(mod))
    eng.close()
    assert g == m
    assert sum(g["alive"][:96]) == 0 and g["info"]["set"] == 0 and g["info"]["fired"] >= 96 and g["counts"]["in_flight"] == 0


# ------------------------------------------------------------------ 10. the refusals, each with its text
def plain_engine(**cfg):
    eng = GpuEngine(EngineConfig(**dict(dict(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1, bucket_actors=32), **cfg)))
    eng.register_range(0, 64, Kind.COUNTER)
    return eng


def test_refuses_without_timers_twice_and_after_the_first_run(built):
    eng = plain_engine()
    assert status_and_text(lambda: eng.set_receive_timeout()) == \
        (EINVAL, "receive timeouts need an engine with timers (agx_set_timers first)")
    eng.set_timers(1)
    eng.set_receive_timeout((4, 5))
    assert status_and_text(lambda: eng.set_receive_timeout()) == \
        (EINVAL, "receive timeouts are set already (agx_set_receive_timeout is called once)")
    assert status_and_text(lambda: eng.set_timers(2)) == \
        (EINVAL, "timers: the key count cannot change once receive timeouts are set (agx_set_receive_timeout)")
    eng.close()
    eng = plain_engine()
    eng.set_timers(1)
    eng.tell(0, 1)
    eng.run()
    assert status_and_text(lambda: eng.set_receive_timeout()) == (ESTATE, "set receive timeouts before the first agx_run")
    eng.close()


def test_inherits_the_timers_refusals(built):
    """no way to an engine with receive timeouts but through agx_set_timers, which refuses max_emit > 1, CRDT kinds,
    other features and more than one rank"""
    eng = plain_engine(max_emit=2)
    assert status_and_text(lambda: eng.set_timers(1))[0] == EINVAL
    assert status_and_text(lambda: eng.set_receive_timeout()) == \
        (EINVAL, "receive timeouts need an engine with timers (agx_set_timers first)")
    eng.close()
    eng = plain_engine()
    eng.set_timers(1)
    eng.set_receive_timeout()
    eng.set_mailbox_class(1, 0)
    assert status_and_text(lambda: eng.set_stash(1, 4))[0] == EINVAL          # (the timers' refusal of another feature)
    assert status_and_text(lambda: eng.set_death_watch(1))[0] == EINVAL
    assert status_and_text(lambda: eng.register_range(0, 8, Kind.GCOUNTER))[0] == EINVAL
    eng.close()


def test_reserved_tag(built):
    eng = plain_engine()
    eng.set_timers(1)
    eng.tell(0, 0xFB000001)  # (without receive timeouts the tag is an ordinary one ...)
    assert status_and_text(lambda: eng.set_receive_timeout()) == \
        (EINVAL, "receive timeouts: a staged tell carries message tag 0xFB, reserved for receive-timeout envelopes")
    eng.close()
    eng = plain_engine()
    eng.set_timers(1)
    eng.set_receive_timeout()
    text = "message tag 0xFB is reserved for receive-timeout envelopes on an engine with receive timeouts"
    assert status_and_text(lambda: eng.tell(0, 0xFB000001)) == (EINVAL, "tell 0: " + text)
    assert status_and_text(lambda: eng.tell_one(0, 0xFB000001)) == (EINVAL, "tell: " + text)
    assert status_and_text(lambda: eng.start_timers(0, 1, 0, 1, payload=0xFB000000)) == (EINVAL, "agx_start_timers: " + text)
    assert status_and_text(lambda: eng.start_receive_timeout(0, 1, 3, 0xFB000000)) == \
        (EINVAL, "agx_start_receive_timeout: message tag 0xFB is reserved for receive-timeout envelopes")
    eng.tell(0, 0xFA000001)
    assert eng.run(1).delivered == 1
    eng.close()


def tagged_tables():
    """tables that name tag 0xFB: no receive timeout in them, so the DSL lets them through"""
    st = typed.State("count", "unused")
    b = (typed.ReceiveBuilder.create(st)
         .on_message(typed.MessageType("Odd", 0xFB), lambda m, s: [s.count.inc(), B.same]).build("names_fb"))
    return typed.compile_behaviors([b], max_emit=1), b


def test_tables_naming_the_reserved_tag(built):
    tb, b = tagged_tables()
    text = "message tag 0xFB"
    for first in ("tables", "feature"):
        eng = GpuEngine(EngineConfig(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1, bucket_actors=32))
        eng.register_range(0, 64, tb.kind_of(b))
        eng.set_timers(1)
        if first == "tables":
            eng.set_behaviors(tb)
            status, msg = status_and_text(lambda: eng.set_receive_timeout())
            assert (status, msg) == (EINVAL, "receive timeouts: the compiled behaviours name message tag 0xFB, reserved for "
                                     "receive-timeout envelopes")
        else:
            eng.set_receive_timeout()
            status, msg = status_and_text(lambda: eng.set_behaviors(tb))
            assert (status, msg) == (EINVAL, "compiled behaviours: message tag 0xFB is reserved for receive-timeout envelopes "
                                     "on an engine with receive timeouts")
        assert text in msg
        eng.close()


def test_tables_and_starts_without_the_feature(built):
    """tables that set or cancel a receive timeout, or agx_start_receive_timeout, on an engine without the feature:
    agx_run returns AGX_EINVAL"""
    w = rc.kat_workload("typed_small_timeout", 5)
    w.timers = {"n_keys": 3}   # (timers, no receive timeouts)
    eng = engine_for(w)
    tell_actor(eng, "Ping")
    assert status_and_text(lambda: eng.run()) == \
        (EINVAL, "the compiled behaviours set or cancel a receive timeout, but the engine has no receive timeouts "
         "(agx_set_receive_timeout)")
    eng.close()
    eng = plain_engine()
    eng.set_timers(1)
    assert status_and_text(lambda: eng.start_receive_timeout(0, 1, 3, 1)) == \
        (EINVAL, "agx_start_receive_timeout needs an engine with receive timeouts (agx_set_receive_timeout)")
    eng.tell(0, 1)
    assert status_and_text(lambda: eng.run()) == \
        (EINVAL, "agx_start_receive_timeout was called on an engine without receive timeouts (agx_set_receive_timeout)")
    eng.set_receive_timeout()   # (the refused start no longer stands in the way)
    eng.start_receive_timeout(0, 1, 3, 1)
    st = eng.run(4)   # (the tell of tick 1 pushes the fire from tick 3 to tick 4)
    info = eng.receive_timeout_info()
    eng.close()
    assert st.delivered == 2 and info == dict(fired=1, discarded=0, set=1, pending=1)


def test_constant_delay_below_one(built):
    """the DSL refuses it (tests/test_typed_receive_timeout.py); tables written by hand are refused by agx_set_behaviors"""
    w = rc.kat_workload("turn_on_in_transparent_handler", 5)
    tb = w.behaviors
    i = next(i for i in range(tb.n_acts) if tb.acts[i].op == typed.A_SET_RECEIVE_TIMEOUT and tb.acts[i].dsrc == typed.V_CONST)
    tb.acts[i].dk = 0
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    status, msg = status_and_text(lambda: eng.set_behaviors(tb))
    eng.close()
    assert status == EINVAL and msg == f"compiled behaviours: action {i} sets a receive timeout of 0 ticks (a constant delay is at least 1)"
