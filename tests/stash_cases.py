"""The scenarios of the stash tests, shared by the CPU file (tests/test_stash_model.py: the model against
the frozen oracle, the reference specs' known answers, the guards that no GPU scenario is vacuous) and
the GPU file (tests/test_gpu_stash.py: the engine against the known answers and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "stash_kats.json").read_text())
TAGS, LETTERS = KATS["tags"], KATS["letters"]
KAT_NAMES = ("support_unstash_all", "unstash_to_returned_behaviors", "stash_while_unstashing", "enforce_capacity")
KAT_T = (1, 3, 5)
N_KAT, ACTOR, HOST = 64, 37, 64
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' (arg a letter of the fixture or a number) -> the u32 payload"""
    name, _, arg = msg.partition(":")
    a = LETTERS[arg] if arg in LETTERS else int(arg or 0)
    return (TAGS[name] << 24) | a


def payloads(msgs) -> np.ndarray:
    return np.asarray([payload(m) for m in msgs], np.uint32)


def kat_behavior(name: str) -> typed.Behavior:
    """The spec's behaviour in the DSL; `processed` is observed as an echo to the host id HOST."""
    host = typed.actor_ref(HOST)
    st = typed.State("count", "last")
    is_ = lambda t: (lambda m: m.tag == TAGS[t])
    B = typed.Behaviors

    def unstash_all_spec(buf):  # StashSpec.scala:33-60 (immutableStash: active / stashing)
        active, stashing = typed.Behavior("active", st), typed.Behavior("stashing", st)
        (typed.ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [s.count.inc(), host.tell(m.payload), B.same], test=is_("Msg"))
         .on_any_message(lambda m, s: [host.tell(s.count, tag=TAGS["GetProcessed"]), B.same], test=is_("GetProcessed"))
         .on_any_message(lambda m, s: [stashing], test=is_("Stash"))
         .on_any_message(lambda m, s: [host.tell(0, tag=TAGS["GetStashSize"]), B.same], test=is_("GetStashSize"))
         .on_any_message(lambda m, s: [B.unhandled])
         .build(into=active))
        (typed.ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [buf.stash(), B.same], test=is_("Msg"))
         .on_any_message(lambda m, s: [buf.stash(), B.same], test=is_("GetProcessed"))
         .on_any_message(lambda m, s: [host.tell(buf.size, tag=TAGS["GetStashSize"]), B.same], test=is_("GetStashSize"))
         .on_any_message(lambda m, s: [buf.unstash_all(active)], test=is_("UnstashAll"))
         .on_any_message(lambda m, s: [B.unhandled])
         .build(into=stashing))
        return active

    def collect_spec(restash_m2: bool):
        def build(buf):  # StashBufferSpec.scala:84-105 / 130-162: stash first, then unstashAll(behavior(""))
            first, collect = typed.Behavior("stash_first", st), typed.Behavior("collect", st)
            (typed.ReceiveBuilder.create(st)
             .on_any_message(lambda m, s: [buf.unstash_all(collect)], test=is_("Go"))
             .on_any_message(lambda m, s: [buf.stash(), B.same])
             .build(into=first))
            rb = typed.ReceiveBuilder.create(st)
            rb.on_any_message(lambda m, s: [host.tell(s.count, tag=TAGS["Get"]), B.same], test=is_("Get"))
            rb.on_any_message(lambda m, s: [buf.unstash_all(B.same)], test=is_("Go"))
            if restash_m2:
                rb.on_any_message(lambda m, s: [buf.stash(), B.same], test=lambda m: m.payload == payload("Msg:m2"))
            rb.on_any_message(lambda m, s: [s.count.inc(), host.tell(m.payload), B.same])
            rb.build(into=collect)
            return first
        return build

    def stash_only(buf):  # StashBufferSpec.scala:55-68
        return (typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [s.count.inc(), buf.stash(), B.same])
                .build("stash_only"))

    cap = KATS[name]["capacity"]
    factory = {"support_unstash_all": unstash_all_spec, "unstash_to_returned_behaviors": collect_spec(False),
               "stash_while_unstashing": collect_spec(True), "enforce_capacity": stash_only}[name]
    return B.with_stash(cap, factory)


def kat_workload(name: str, T: int) -> wl.Workload:
    b = kat_behavior(name)
    tb = typed.compile_behaviors([b], max_emit=1)
    w = wl.Workload("stash_kat", N_KAT, 2, 1, T, 0, [(0, N_KAT, tb.kind_of(b), None)], behaviors=tb,
                    outbound=(HOST, 1), bucket_actors=32, stash={0: tb.stash_capacity})
    return w


def tell_script(target, msgs):
    p = payloads(msgs)
    target.tell(np.full(p.size, ACTOR, np.uint32), p, np.full(p.size, NO_SENDER, np.uint32))


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def run_kat(name: str, T: int, target) -> dict:
    """Run the spec's script on `target` (an engine or the model, the workload applied): what the tests
    compare -- echoes, the actor's stash, the stash totals and the counters after each part."""
    k = KATS[name]
    out = {}
    for part, script in (("", k["script"]), ("second_", k.get("second_script"))):
        if script is None:
            continue
        tell_script(target, script)
        st = counts(target.run())
        s, p, rel = target.read_stash(ACTOR)
        out[part + "echo"] = target.take_outbound()[2].tolist()
        out[part + "stash"] = p.tolist()
        out[part + "released"] = rel
        out[part + "info"] = target.stash_info()
        out[part + "counts"] = st
        out[part + "alive"] = int(target.read_state()[1][ACTOR])
    return out


def check_kat(name: str, got: dict):
    k = KATS[name]
    for part in ("", "second_") if "second_script" in k else ("",):
        assert got[part + "echo"] == payloads(k[part + "expected"]).tolist(), (part, got[part + "echo"])
        assert got[part + "stash"] == payloads(k[part + "final_stash"]).tolist()
        assert got[part + "released"] == 0 and got[part + "info"]["pending"] == 0
        info, st = got[part + "info"], got[part + "counts"]
        assert info["stashed"] == k[part + "stashed"] and info["unstashed"] == k[part + "unstashed"]
        assert info["overflows"] == k["overflows"] and info["held"] == len(k[part + "final_stash"])
        assert st["delivered"] == k[part + "delivered"] and st["dead_letters"] == k.get("dead_letters", 0)
        assert st["in_flight"] == info["held"]
        assert st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]
        assert got[part + "alive"] == (0 if k.get("stopped") else 1)


# ---- a small population for the pending-only / held-only / stop scenarios: 101 gates, 32-actor buckets
N_SMALL, SMALL_BUCKET, SMALL_S, LAST = 101, 32, 4, 99   # actor 99 lives in the partial last bucket


def small_gates(T: int = 1, classes: dict | None = None, mailboxes=(), stash=None, hop: int = 0) -> wl.Workload:
    """101 closed gates (wl.gate) on class 0 with a stash of SMALL_S; host id 101 is the observer."""
    closed, opened = wl.gate(N_SMALL, SMALL_S, hop or wl.STASH_GATE_HOP)
    tb = typed.compile_behaviors([closed, opened], max_emit=1)
    return wl.Workload("small_gates", N_SMALL, 2, 1, T, 0, [(0, N_SMALL, tb.kind_of(closed), None)], behaviors=tb,
                       outbound=(N_SMALL, 1), bucket_actors=SMALL_BUCKET, mailbox_classes=dict(classes or {}),
                       mailboxes=list(mailboxes), stash={0: SMALL_S} if stash is None else stash)


def gate_msgs(tag: int, args, dst: int = LAST):
    """(dst, payload, src): messages from the host-side observer (an open gate echoes them back)"""
    p = (np.uint32(tag) << np.uint32(24)) | np.asarray(args, np.uint32)
    return np.full(p.size, dst, np.uint32), p, np.full(p.size, N_SMALL, np.uint32)


# ---- a stop with a non-empty buffer and park (unstashRestToDeadLetters)
STOP_TAG = 9


def stop_workload(T: int = 3) -> wl.Workload:
    """One actor that stashes everything (a Stop too) until Go, then echoes Msg and stops on Stop."""
    host, st, B = typed.actor_ref(HOST), typed.State("count", "last"), typed.Behaviors

    def build(buf):
        first, second = typed.Behavior("stash_first", st), typed.Behavior("stop_on_stop", st)
        (typed.ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [buf.unstash_all(second)], test=lambda m: m.tag == TAGS["Go"])
         .on_any_message(lambda m, s: [buf.stash(), B.same])
         .build(into=first))
        (typed.ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [B.stopped], test=lambda m: m.tag == STOP_TAG)
         .on_any_message(lambda m, s: [s.count.inc(), host.tell(m.payload), B.same])
         .build(into=second))
        return first

    b = B.with_stash(6, build)
    tb = typed.compile_behaviors([b], max_emit=1)
    return wl.Workload("stash_stop", N_KAT, 2, 1, T, 0, [(0, N_KAT, tb.kind_of(b), None)], behaviors=tb,
                       outbound=(HOST, 1), bucket_actors=32, stash={0: 6})


def stop_script(target) -> dict:
    """T = 3, all staged at once: [m1 Stop m2] and m3 are stashed, Go releases the four and parks m4 (m5 stays
    queued); the released window echoes m1 and stops on Stop with m2, m3 buffered and m4 parked."""
    p = payloads(["Msg:m1"]).tolist() + [STOP_TAG << 24] + payloads(["Msg:m2", "Msg:m3", "Go", "Msg:m4", "Msg:5"]).tolist()
    p = np.asarray(p, np.uint32)
    target.tell(np.full(p.size, ACTOR, np.uint32), p, np.full(p.size, NO_SENDER, np.uint32))
    target.run(2)
    mid = target.stash_info()
    st = counts(target.run())
    return dict(mid=mid, counts=st, info=target.stash_info(), echo=target.take_outbound()[2].tolist(),
                alive=int(target.read_state()[1][ACTOR]))


# ---- population parity: (seed, throughput) of wl.stash_gate(2048, ...); see test_stash_model.py's guards
POPULATION = [(1, 3), (4, 5)]
POPULATION_BUCKETS = (128,)   # (at 2048 the population is one bucket: no "bucket of pending actors only" there)
TILE = 2048
