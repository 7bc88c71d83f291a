"""The scenarios of the ask tests, shared by the CPU file (tests/test_ask_model.py: the model against the reference
specs' known answers and the rules of DESIGN.md §2.9) and the GPU file (tests/test_gpu_ask.py: the engine against
the known answers and, snapshot for snapshot, the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER, Kind

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "ask_kats.json").read_text())
TAGS = KATS["tags"]
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 4)
# 80 actors in buckets of 32 (a partial last bucket).  The snitch asks; FLOOD < TARGET (its tells arrive first);
# TARGET sits in another bucket than the snitch, NEAR in the snitch's own; MISSING is no actor and no host id
N_KAT, ACTOR, HOST = 80, 37, 80
FLOOD, TARGET, NEAR, MISSING = 2, 5, 40, 200
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
ASK_KEYS = ("asked", "answered", "timed_out", "late")
NONE = 0xFFFFFFFF
B = typed.Behaviors


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload"""
    name, _, arg = msg.partition(":")
    return (TAGS[name] << 24) | int(arg or 0)


def mtype(name: str) -> typed.MessageType:
    return typed.MessageType(name, TAGS[name])


def snitch(timeout: int) -> typed.Behavior:
    """The asking actor of ActorContextAskSpec, driven by messages.  State word 1 is the target's id, word 0 counts
    what came back.  Ask0..Ask3(n) ask Ping(n) on keys 0..3 with the reply mapped to Adapted; AskRaw(n) asks on key
    0 without a mapping; AskSelf asks the actor itself.  Adapted, Pong and TimedOut are echoed to the host id HOST (a
    Pong whose sender is not the actor itself as Pong(0xBAD): the behaviour sees sender = self on a reply).
    Cancel cancels key 0, CancelAll all keys; Plain(d) starts a plain single timer of d ticks on key 1 (PlainFired
    is echoed); Pending echoes IsPending(1 or 0) for key 0; Noop does nothing; Ping(n) is answered with Pong(n), as a
    replier does; Stop stops."""
    host = typed.actor_ref(HOST)
    st = typed.State("got", "target")
    ctx = typed.context
    keys = ("k0", "k1", "k2", "k3")

    def build(timers):
        for k in keys:
            timers.cancel(k)  # (the keys, in slot order)
        rb = typed.ReceiveBuilder.create(st)
        for i, k in enumerate(keys):
            rb.on_message(mtype(f"Ask{i}"), lambda m, s, k=k: [
                ctx.ask(s.target.ref, mtype("Ping")(m.arg), timeout, on_timeout=mtype("TimedOut")(), on_success=mtype("Adapted"), key=k),
                B.same])
        return (rb.on_message(mtype("AskRaw"), lambda m, s: [
                    ctx.ask(s.target.ref, mtype("Ping")(m.arg), timeout, on_timeout=mtype("TimedOut")(), key="k0"), B.same])
                .on_message(mtype("AskSelf"), lambda m, s: [
                    ctx.ask(typed.self_ref(), mtype("Ping")(m.arg), timeout, on_timeout=mtype("TimedOut")(),
                            on_success=mtype("Adapted"), key="k0"), B.same])
                .on_message(mtype("Adapted"), lambda m, s: [s.got.inc(), host.tell(mtype("Adapted")(m.arg)), B.same])
                .on_message(mtype("Pong"), lambda m, s: [s.got.inc(), host.tell(mtype("Pong")(m.arg)), B.same],
                            when=lambda m, s: typed.Operand(typed.V_SENDER) == typed.Operand(typed.V_SELF))
                .on_message(mtype("Pong"), lambda m, s: [s.got.inc(), host.tell(mtype("Pong")(0xBAD)), B.same])
                .on_message(mtype("TimedOut"), lambda m, s: [s.got.inc(), host.tell(mtype("TimedOut")()), B.same])
                .on_message(mtype("Cancel"), lambda m, s: [timers.cancel("k0"), B.same])
                .on_message(mtype("CancelAll"), lambda m, s: [timers.cancel_all(), B.same])
                .on_message(mtype("Plain"), lambda m, s: [timers.start_single_timer("k1", mtype("PlainFired")(), m.arg), B.same])
                .on_message(mtype("PlainFired"), lambda m, s: [host.tell(mtype("PlainFired")()), B.same])
                .on_message(mtype("Pending"), lambda m, s: [host.tell(mtype("IsPending")(1)), B.same],
                            when=lambda m, s: ctx.ask_pending("k0"))
                .on_message(mtype("Pending"), lambda m, s: [host.tell(mtype("IsPending")(0)), B.same])
                .on_message(mtype("Noop"), lambda m, s: [B.same])
                .on_message(mtype("Ping"), lambda m, s: [m.sender.tell(mtype("Pong")(m.arg)), B.same])
                .on_message(mtype("Stop"), lambda m, s: [B.stopped])
                .on_any_message(lambda m, s: [B.unhandled])
                .build("snitch"))
    return B.with_timers(build)


def target_behavior(kind: str) -> typed.Behavior:
    """replier: Ping(n) -> Pong(n) to the sender (the ask ref), Stop stops.  ignore: Behaviors.ignore.  empty:
    Behaviors.empty (everything unhandled).  keeper: the first Ping stores its sender in word 1, Answer(n) tells that ref
    Pong(n).  flooder: Poke tells the snitch Noop."""
    st = typed.State("n", "ref")
    rb = typed.ReceiveBuilder.create(st)
    if kind == "replier":
        rb.on_message(mtype("Ping"), lambda m, s: [s.n.inc(), m.sender.tell(mtype("Pong")(m.arg)), B.same])
        rb.on_message(mtype("Stop"), lambda m, s: [B.stopped])
    elif kind == "ignore":
        return rb.on_any_message(lambda m, s: [B.same]).build("ignore")
    elif kind == "keeper":  # (it keeps the first sender only)
        rb.on_message(mtype("Ping"), lambda m, s: [s.n.inc(), s.ref.set(m.sender.dst), B.same], when=lambda m, s: s.ref == 0)
        rb.on_message(mtype("Ping"), lambda m, s: [s.n.inc(), B.same])
        rb.on_message(mtype("Answer"), lambda m, s: [s.ref.ref.tell(mtype("Pong")(m.arg)), B.same])
    elif kind == "flooder":
        rb.on_message(mtype("Poke"), lambda m, s: [typed.actor_ref(ACTOR).tell(mtype("Noop")()), B.same])
    return rb.on_any_message(lambda m, s: [B.unhandled]).build(kind)


def ask_workload(timeout: int, T: int, target: str = "replier", target_id: int = TARGET, askers=((ACTOR, 1),),
                 capacity: int = 0, pingpong: bool = False) -> wl.Workload:
    """N_KAT actors: `askers` ranges of snitches whose target is `target_id` (None: actor i asks actor (i + 40)
    mod 80), FLOOD a flooder, every other actor a `target` behaviour (a PingPong of the fixed kind with
    `pingpong`).  The snitches' mailbox has `capacity` (0: unbounded)."""
    sn = snitch(timeout)
    behs = {k: target_behavior(k) for k in {target, "flooder"} - {"missing", "stopped"} | {"replier"}}
    tb = typed.compile_behaviors([sn] + [behs[k] for k in sorted(behs)], max_emit=1)
    assert tb.uses_ask and tb.timer_keys == 4
    tk = "replier" if target in ("missing", "stopped") else target
    kind = np.full(N_KAT, int(Kind.PINGPONG) if pingpong else tb.kind_of(behs[tk]), np.int64)
    init = np.zeros((N_KAT, 2), np.uint64)
    if pingpong:
        init[:, 0] = 1 << 40  # (a PingPong stops when word 0 reaches 0: never here)
    kind[FLOOD] = tb.kind_of(behs["flooder"])
    for first, count in askers:
        kind[first:first + count] = tb.kind_of(sn)
        init[first:first + count, 0] = 0
        init[first:first + count, 1] = target_id if target_id is not None else (np.arange(first, first + count) + 40) % N_KAT
    cuts = [0] + [i for i in range(1, N_KAT) if kind[i] != kind[i - 1]] + [N_KAT]
    ranges = [(f, t - f, int(kind[f]), init[f:t].copy()) for f, t in zip(cuts, cuts[1:])]
    return wl.Workload("ask_kat", N_KAT, 2, 1, T, 0, ranges, behaviors=tb, outbound=(HOST, 1), bucket_actors=32,
                       mailbox_classes={1: capacity} if capacity else {},
                       mailboxes=[(f, c, 1) for f, c in askers] if capacity else [],
                       timers={"n_keys": 4, "ask": True})


def kat_workload(name: str, T: int) -> wl.Workload:
    su = SCENARIOS[name]["setup"]
    return ask_workload(su["timeout"], T, su["target"], MISSING if su["target"] == "missing" else TARGET)


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def conserved(st: dict, timer_info: dict) -> bool:
    """the timers' own: staged + emitted + fired = delivered + dead_letters + in_flight"""
    return st["staged"] + st["emitted"] + timer_info["fired"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def tell(target, *msgs, actor=ACTOR):
    p = np.asarray([payload(m) for m in msgs], np.uint32)
    target.tell(np.full(p.size, actor, np.uint32), p, np.full(p.size, NO_SENDER, np.uint32))


def per_sender(d, s, p):
    """the outbox as [src], [dst], [payload] in canonical order: by sender, each sender's messages in its order"""
    o = np.argsort(s, kind="stable")
    return [s[o].tolist(), d[o].tolist(), p[o].tolist()]


def snapshot(target, st) -> dict:
    """everything observable: counters, both infos, every slot of every actor, state words, alive flags, the outbox"""
    st = counts(st)
    ti, ai = target.timer_info(), target.ask_info()
    assert conserved(st, ti), (st, ti)
    slots = []
    for a in range(N_KAT):
        t, k = target.read_timers(a), target.read_asks(a)
        slots.append([t[f].tolist() for f in ("active", "remaining", "period", "payload", "generation")] +
                     [k[f].tolist() for f in ("is_ask", "adapt")])
    words, alive = target.read_state()
    return dict(counts=st, timer_info=ti, info=ai, slots=slots, words=words.tolist(), alive=(alive & 1).tolist(),
                echo=per_sender(*target.take_outbound()))


def echoes(snap) -> list:
    """the payloads the snitch ACTOR echoed, in order"""
    return [p for s, p in zip(snap["echo"][0], snap["echo"][2]) if s == ACTOR]


def run_kat(name: str, T: int, target) -> dict:
    """Run the scenario on `target` (an engine or the model, the workload applied): the echoes, the ticks the scenario
    took, the final counters and infos."""
    sc = SCENARIOS[name]
    if sc["setup"]["target"] == "stopped":  # (the target has terminated before the ask)
        tell(target, "Stop", actor=TARGET)
        target.run()
    t0 = target.timer_info()["ticks"]
    tell(target, *sc["tell"])
    st = counts(target.run())
    ti, ai = target.timer_info(), target.ask_info()
    assert conserved(st, ti), (name, T, st, ti)
    d, s, p = target.take_outbound()
    assert (d == HOST).all() and (s == ACTOR).all()
    words, alive = target.read_state()
    return dict(echo=[int(x) for x in p], ticks=ti["ticks"] - t0, counts=st, info=ai, timer_info=ti,
                got=int(words[ACTOR, 0]), alive=int(alive[ACTOR] & 1), slots=[target.read_timers(ACTOR)["active"].tolist(),
                                                                              target.read_asks(ACTOR)["is_ask"].tolist()])


def per_T(v, T: int):
    """a value of the JSON that differs by throughput is written {"1": .., "4": ..}"""
    return v[str(T)] if isinstance(v, dict) and set(v) == {"1", "4"} else v


def check_kat(name: str, T: int, got: dict) -> None:
    """`got` against the JSON."""
    sc = SCENARIOS[name]
    assert got["echo"] == [payload(m) for m in sc["echo"]], (got["echo"], sc["echo"])
    assert got["ticks"] == per_T(sc["ticks"], T), (got["ticks"], sc["ticks"])
    f = sc["final"]
    assert got["info"] == {k: f[k] for k in ASK_KEYS}, got["info"]
    assert got["counts"]["dead_letters"] == f["dead_letters"] and got["counts"]["unhandled"] == f["unhandled"], got["counts"]
    assert got["timer_info"]["fired"] == f["fired"] and got["timer_info"]["discarded"] == f["discarded"], got["timer_info"]
    assert got["counts"]["in_flight"] == 0 and got["timer_info"]["pending"] == 0 and got["timer_info"]["active"] == 0
    assert got["got"] == len(sc["echo"]) and got["alive"] == 1 and got["slots"] == [[0] * 4, [0] * 4]


# ------------------------------------------------------------------ one case per rule of DESIGN.md §2.9
# Each takes make(workload) -> target and returns the snapshots it took; expectations that the model test asserts are
# in EXPECT (functions of the snapshots).  The GPU test compares engine and model snapshot for snapshot.
def P(m):
    return payload(m)


def _script(make, w, steps):
    """steps: (tells [(actor, msg, ...)], budget or None) -> a snapshot after each"""
    t = make(w)
    out = []
    for tells, budget in steps:
        for actor, *msgs in tells:
            tell(t, *msgs, actor=actor)
        out.append(snapshot(t, t.run() if budget is None else t.run(budget)))
    t.close()
    return out


def case_reply_and_timeout_in_one_tick(make, T):
    """t = 2 against a prompt target: the reply and the TimerMsg are in the inbox of tick 3, the reply first -- it wins"""
    return _script(make, ask_workload(2, T), [([(ACTOR, "Ask0:5")], None)])


def case_t1_against_prompt_target(make, T):
    """t = 1 always times out: the timeout comes in tick 2, the reply in tick 3 and is late"""
    return _script(make, ask_workload(1, T), [([(ACTOR, "Ask0:5")], None)])


def case_late_reply_after_timeout(make, T):
    """the keeper answers after the timeout: late, the behaviour does not run, not unhandled"""
    return _script(make, ask_workload(2, T, "keeper"), [([(ACTOR, "Ask0:5")], None), ([(TARGET, "Answer:9")], None)])


def case_two_replies(make, T):
    """two replies to one ask: the second is late"""
    return _script(make, ask_workload(9, T, "keeper"), [([(ACTOR, "Ask0:5")], 2), ([(TARGET, "Answer:1", "Answer:2")], None)])


def case_supersede(make, T):
    """asking again on the key supersedes: the first reply is of another generation and late, the second accepted"""
    return _script(make, ask_workload(9, 1), [([(ACTOR, "Ask0:1", "Ask0:2")], None)])


def case_cancel(make, T):
    """timers.cancel(k) abandons the ask: its reply is late, no timeout comes"""
    return _script(make, ask_workload(5, 1), [([(ACTOR, "Ask0:1", "Cancel")], None)])


def case_cancel_all(make, T):
    return _script(make, ask_workload(5, 1), [([(ACTOR, "Ask0:1", "Ask1:2", "CancelAll")], None)])


def case_asker_stops(make, T):
    """a stop of the asker cancels its slots; the reply is an ordinary dead letter"""
    return _script(make, ask_workload(5, 1), [([(ACTOR, "Ask0:1", "Stop")], None)])


def case_keeper_answers_later(make, T):
    """the target stores the ref and answers three ticks later: accepted, adapted"""
    return _script(make, ask_workload(9, T, "keeper"), [([(ACTOR, "Ask0:5")], 5), ([(TARGET, "Answer:6")], None)])


def case_full_mailbox_kills_reply(make, T):
    """the snitch's mailbox holds one message: the flooder's Noop (from a lower id: first) takes the slot of tick 3,
    the reply dies at admission and the timeout follows"""
    return _script(make, ask_workload(4, T, capacity=1), [([(ACTOR, "Ask0:5")], 1), ([(FLOOD, "Poke")], None)])


def case_ask_and_plain_timer(make, T):
    """an ask on key 0 and a plain timer on key 1: the reply is accepted, the plain timer fires, nothing timed out"""
    return _script(make, ask_workload(6, T), [([(ACTOR, "Plain:4", "Ask0:5")], None)])


def case_reply_to_plain_timer_slot(make, T):
    """Ask1 on key 1 (the keeper keeps the ref), then 128 plain starts on key 1: the slot is active with the ref's
    generation mod 2^7 but no ask's -- the reply is late"""
    return _script(make, ask_workload(400, 4, "keeper"),
                   [([(ACTOR, "Ask1:5")], 2), ([(ACTOR, *["Plain:300"] * 128)], 40), ([(TARGET, "Answer:6")], 4)])


def case_generation_alias(make, T):
    """bounded difference 4: 128 further asks on the key while the first reply is outstanding -- the keeper's reply
    to the first ask agrees mod 2^7 with the 129th and is accepted for it"""
    return _script(make, ask_workload(400, 4, "keeper"),
                   [([(ACTOR, "Ask0:5")], 2), ([(ACTOR, *["Ask0:7"] * 128)], 40), ([(TARGET, "Answer:6")], 4)])


def case_ask_pending(make, T):
    """ask_pending reads 1 while the ask is outstanding and 0 once answered"""
    return _script(make, ask_workload(9, 1, "keeper"),
                   [([(ACTOR, "Ask0:5", "Pending")], 3), ([(TARGET, "Answer:6")], None), ([(ACTOR, "Pending")], None)])


def case_ask_self(make, T):
    """an actor that asks itself: the request names the receiver, so it is its own reply"""
    return _script(make, ask_workload(5, T), [([(ACTOR, "AskSelf:3")], None)])


def case_same_bucket(make, T):
    """asker and target in one bucket"""
    return _script(make, ask_workload(3, T, target_id=NEAR), [([(ACTOR, "Ask0:5")], 1), ([], 1), ([], None)])


def case_two_buckets(make, T):
    """asker and target in two buckets, tick by tick"""
    return _script(make, ask_workload(3, T), [([(ACTOR, "Ask0:5")], 1), ([], 1), ([], None)])


def case_all_ask(make, T):
    """all 80 actors ask in one tick, actor i asks actor (i + 40) mod 80, and all answer"""
    w = ask_workload(4, T, askers=((0, N_KAT),), target_id=None)
    return _script(make, w, [([(a, f"Ask{a % 4}:{a}") for a in range(N_KAT)], 1), ([], 1), ([], None)])


def case_pingpong_target(make, T):
    """a fixed-kind target (AGX_KIND_PINGPONG answers its sender) answers an ask too"""
    return _script(make, ask_workload(3, T, pingpong=True), [([(ACTOR, "AskRaw:5")], None)])


def case_timeout_only_bucket(make, T):
    """the partial last bucket's only work is an ask's timeout: actor 70 asks a missing target"""
    w = ask_workload(6, T, "missing", MISSING, askers=((70, 1),))
    return _script(make, w, [([(70, "Ask0:5")], 1), ([], 3), ([], None)])


RULE_CASES = {f.__name__[5:]: f for f in (
    case_reply_and_timeout_in_one_tick, case_t1_against_prompt_target, case_late_reply_after_timeout, case_two_replies,
    case_supersede, case_cancel, case_cancel_all, case_asker_stops, case_keeper_answers_later,
    case_full_mailbox_kills_reply, case_ask_and_plain_timer, case_reply_to_plain_timer_slot, case_generation_alias,
    case_ask_pending,
    case_ask_self, case_same_bucket, case_two_buckets, case_all_ask, case_pingpong_target, case_timeout_only_bucket)}
