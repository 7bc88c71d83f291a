"""The conformance program of the compiled-behaviour rule (DESIGN.md §8 "The compiled rule at 64-bit edges"): one
population of N = 465 actors that walks the rule of include/akka_gpu.h "compiled behaviours" through its 64-bit edges.

Layout (ids):
  0                 a V_SELF probe (behaviour `selfdk`)
  1 .. 7            sinks
  8 .. 207          probes (P = 200 places): each receives a short FIFO script of host tells of its own
  208 .. 223        sinks around the V_SELF probe 216, a mid id: every small dk reaches a sink without a wrap
  224 .. 423        recorders: everything probe p sends goes to p + R, R = 216, through the sender operand (the host tells
                    carry the recorder's id as their sender) or through (self + R) mod n
  424 .. 427        never registered (the entity range / child block of the sharding and children variants)
  428 .. N - 2      sinks
  N - 1             a V_SELF probe

A recorder has one sender, so its state depends on no cross-actor order: word 0 += 2^40 + payload (a count in the high
bits, the sum of the payloads below), word 1 = sender << 32 | payload of the last envelope (the shift is 32 doublings:
every recorded envelope also runs "an action reads what an earlier one wrote" and a carry across 2^32).  Sinks and
V_SELF probes record commutatively (word 0 += 2^40 + payload, word 1 += 2^48 + sender): the (self + dk) mod n cases
reach them from more than one sender.

N divides 2^40 - 1, so (2^40 + 5) mod N = 6 while the same sum cut to 32 bits gives 5; N is odd and no multiple of any
tile.  Every named case is one probe: CASES lists them."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER
from tests import compiled_core_model as core

N = 465
HEAD = 8
P = 200
MID0, MID_N = HEAD + P, 16     # the sinks in the middle
R = P + MID_N                  # a probe's recorder is R ids on
HOLE0, HOLE_N = HEAD + P + R, 4
S_IDS = (0, MID0 + MID_N // 2, N - 1)
M64 = (1 << 64) - 1
REC = "REC"  # a script's sender / an initial word: the probe's recorder id
B = typed.Behaviors
ST = typed.State("a", "b")
W0, W1 = ST.a, ST.b


def H(hi, lo):
    return (hi << 32) | lo


def O(src, word=0, k=0):
    return typed.Operand(src, word, k)


def const(v):
    """the constant v (0 .. 2^64 - 1) as an operand: k is a signed 64-bit field"""
    return O(typed.V_CONST, 0, v if v < (1 << 63) else v - (1 << 64))


PAY, TAG, ARG, SENDER = O(typed.V_PAYLOAD), O(typed.V_TAG), O(typed.V_ARG), O(typed.V_SENDER)
TO_REC = O(typed.V_SELF, 0, R)  # (self + R) mod n: the probe's recorder


def T(cmp, a, b):
    return typed.Test(cmp, typed.lift(a), typed.lift(b))


def tell(dst, val, mask=0):
    return typed.Action(typed.A_TELL, 0, typed.lift(val), dst, mask)


def beh(name, *cases, into=None):
    """a behaviour of (tests, effects, result) cases, through the DSL's ReceiveBuilder"""
    rb = typed.ReceiveBuilder.create(ST)
    for tests, effects, result in cases:
        t1 = tests[0] if len(tests) > 0 else None
        t2 = tests[1] if len(tests) > 1 else None
        rb.on_any_message(lambda m, s, e=effects, r=result: list(e) + [r],
                          test=(lambda m, t=t1: t) if t1 is not None else None,
                          when=(lambda m, s, t=t2: t) if t2 is not None else None)
    return rb.build(name, into=into)


def tag_is(j):
    return T(typed.CMP_EQ, TAG, j)


# ------------------------------------------------------------------ the behaviours
DKS = (0, 1, -1, N, -N, N + 3, -(N + 3), (1 << 40) + 5, -((1 << 40) + 5))
SRCS = (("const", typed.V_CONST, 0), ("payload", typed.V_PAYLOAD, 0), ("tag", typed.V_TAG, 0), ("arg", typed.V_ARG, 0),
        ("word0", typed.V_WORD, 0), ("word1", typed.V_WORD, 1), ("sender", typed.V_SENDER, 0), ("self", typed.V_SELF, 0))
KS = (0, 1, -1, 1 << 31, 1 << 32, -(1 << 32), (1 << 63) - 1, -(1 << 63))
PAIRS = (("0_max", 0, M64), ("s31", (1 << 31) - 1, 1 << 31), ("s32", (1 << 32) - 1, 1 << 32), ("s63", (1 << 63) - 1, 1 << 63),
         ("eq_hi", (1 << 63) + 5, (1 << 63) + 5), ("lo_eq", H(1, 7), H(2, 7)), ("cross", H(1, 9), H(2, 3)))
ORIENTED = tuple((f"{n}{'' if i == 0 else '_rev'}", *(p if i == 0 else p[::-1])) for n, *p in PAIRS for i in (0, 1))
SEL = H(0x77, 0x10)
SINK_FX = [W0.add(O(typed.V_PAYLOAD, 0, 1 << 40)), W1.add(O(typed.V_SENDER, 0, 1 << 48))]
ACT_FX = {  # tag -> (name, tests beside the tag, effects, the word the case then tells)
    1: ("set0_arg_hi", [], [W0.set(O(typed.V_ARG, 0, 1 << 33))], W0),
    2: ("set1_negative_k", [], [W1.set(O(typed.V_ARG, 0, -(1 << 33)))], W1),
    3: ("add0_one", [], [W0.add(1)], W0),
    4: ("add1_one", [], [W1.add(1)], W1),
    5: ("add0_minus_one", [], [W0.add(-1)], W0),
    6: ("add1_minus_2p32", [], [W1.add(-(1 << 32))], W1),
    7: ("max0_word1", [], [W0.max(W1)], W0),
    8: ("max1_word0", [], [W1.max(W0)], W1),
    9: ("min0_word1", [], [W0.min(W1)], W0),
    10: ("min1_word0", [], [W1.min(W0)], W1),
    11: ("max0_2p63", [], [W0.max(const(1 << 63))], W0),
    12: ("min1_2p63", [], [W1.min(const(1 << 63))], W1),
    13: ("max0_itself", [], [W0.max(W0)], W0),
    14: ("min1_itself", [], [W1.min(W1)], W1),
    15: ("later_reads_earlier", [], [W0.set(ARG), W1.add(W0), W0.add(W1)], W0),
    16: ("tell_after_set", [], [W0.set(O(typed.V_ARG, 0, 5))], W0),
    17: ("guard_sees_old", [T(typed.CMP_GE, W0, const(1 << 32))], [W0.set(3)], W0),
    18: ("add0_itself", [], [W0.add(W0)], W0),
    19: ("add1_itself", [], [W1.add(W1)], W1),
    20: ("min0_arg", [], [W0.min(ARG)], W0),
    21: ("max1_arg_2p63", [], [W1.max(O(typed.V_ARG, 0, (1 << 63) - 1))], W1),
}
ACT_STATES = {"carry": (H(1, 0xFFFFFFFF), M64), "sign": ((1 << 63) - 1, 1 << 63), "equal": ((1 << 63) + 9, (1 << 63) + 9),
              "cross": (H(5, 3), H(3, 5))}


@functools.lru_cache(maxsize=None)
def behaviors():
    """name -> Behavior (built once: the tables of both programs hold the same objects)"""
    b = {}
    b["recorder"] = beh("recorder", ([], [W0.add(O(typed.V_PAYLOAD, 0, 1 << 40)), W1.set(SENDER)] + [W1.add(W1)] * 32 +
                                     [W1.add(PAY)], B.same))
    b["sink"] = beh("sink", ([], SINK_FX, B.same))
    b["selfdk"] = beh("selfdk", *[([tag_is(j)], [tell(O(typed.V_SELF, 0, dk), ARG, 0x20 << 24)], B.same)
                                  for j, dk in enumerate(DKS, 1)], ([tag_is(0x20)], SINK_FX, B.same))
    cases = []
    for si, (_, src, word) in enumerate(SRCS):
        for ki, k in enumerate(KS):
            cases.append(([tag_is(1 + si * 8 + ki)], [W0.set(O(src, word, k)), W1.add(W0), tell(TO_REC, W0)], B.same))
    b["opnd"] = beh("opnd", *cases)
    b["pay"] = beh("pay", ([], [W0.set(PAY), W1.add(O(typed.V_TAG, 0, 1 << 32)), W1.add(ARG),
                                tell(SENDER, O(typed.V_PAYLOAD, 0, 1))], B.same))
    hit, miss = [tell(SENDER, O(typed.V_TAG, 0, 0x100))], ([], [tell(SENDER, TAG)], B.same)
    b["cmpww"] = beh("cmpww", *[([tag_is(c), T(c, W0, W1)], hit, B.same) for c in range(1, 7)], miss)
    b["cmpww_r"] = beh("cmpww_r", *[([T(c, W0, W1), tag_is(c)], hit, B.same) for c in range(1, 7)], miss)
    b["cmpwc"] = beh("cmpwc", *[([tag_is(1 + pi * 6 + c - 1), T(c, W0, const(rhs))], hit, B.same)
                                for pi, (_, _, rhs) in enumerate(ORIENTED) for c in range(1, 7)], miss)
    b["cmppw"] = beh("cmppw", *[([T(typed.CMP_EQ, W1, const(SEL + c)), T(c, PAY, W0)],
                                 [W1.add(1), tell(TO_REC, W1)], B.same) for c in range(1, 7)],
                     ([], [W1.add(1), tell(TO_REC, 0)], B.same))
    b["act"] = beh("act", *[([tag_is(j)] + tests, fx + [tell(SENDER, word)], B.same)
                            for j, (_, tests, fx, word) in ACT_FX.items()], miss)
    b["fm"] = beh("fm", ([T(typed.CMP_GE, ARG, 10)], [W0.add(1), tell(SENDER, W0)], B.same),
                  ([T(typed.CMP_GE, ARG, 5)], [W0.add(1 << 16), tell(SENDER, W0)], B.same),
                  ([], [W0.add(1 << 32), tell(SENDER, W0)], B.same))
    b["nomatch"] = beh("nomatch", ([T(typed.CMP_EQ, ARG, 99)], [W0.add(1)], B.same))
    b["empty"] = beh("empty")
    b["unh_act"] = beh("unh_act", ([tag_is(9)], [W0.add(7), tell(SENDER, W0)], B.unhandled), ([], [W1.add(1)], B.same))
    b["stop_act"] = beh("stop_act", ([tag_is(2)], [W1.set(ARG), tell(SENDER, O(typed.V_ARG, 0, 1))], B.stopped),
                        ([], [W0.add(ARG)], B.same))
    cA, cB, cC = (typed.Behavior(f"chain{x}", ST) for x in "ABC")
    beh("chainA", ([tag_is(1)], [W0.add(1)], cB), ([], [W1.add(ARG)], B.same), into=cA)
    beh("chainB", ([tag_is(1)], [W0.add(1 << 32)], cC), ([], [W1.add(O(typed.V_ARG, 0, 1 << 40))], B.same), into=cB)
    beh("chainC", ([tag_is(1)], [W0.add(1 << 48)], cA), ([], [W1.set(ARG)], B.same), into=cC)
    b["chainA"], b["chainB"], b["chainC"] = cA, cB, cC
    sb = typed.Behavior("selfbecome", ST)
    b["selfbecome"] = beh("selfbecome", ([tag_is(1)], [W0.add(1)], sb), ([], [W1.add(ARG)], B.same), into=sb)
    b["wdst"] = beh("wdst", ([], [W1.add(1), tell(O(typed.V_WORD, 0), ARG)], B.same))
    b["sdst"] = beh("sdst", ([tag_is(1)], [W0.add(1 << 32), tell(O(typed.V_SENDER, 0, 1), ARG)], B.same),
                    ([], [W0.add(1), tell(SENDER, ARG)], B.same))
    zero = typed.MessageType("Zero", 0)
    b["mask"] = beh("mask", ([tag_is(1)], [tell(SENDER, W0, 0x55 << 24)], B.same), ([tag_is(2)], [tell(SENDER, W0)], B.same),
                    ([tag_is(3)], [typed.Ref(SENDER).tell(zero(W0))], B.same), ([tag_is(4)], [tell(SENDER, W1, 1)], B.same))
    b["two"] = beh("two", ([tag_is(1)], [tell(SENDER, W0), W0.add(1), tell(SENDER, W0)], B.same),
                   ([], [tell(SENDER, ARG), tell(SENDER, O(typed.V_ARG, 0, 1)), W0.add(1)], B.same))
    return b


# ------------------------------------------------------------------ the named cases
@dataclasses.dataclass
class Probe:
    name: str
    beh: str          # a behaviour's name; "badkind": a kind past the tables' behaviours
    w0: object
    w1: object
    script: list      # (sender, payload); REC stands for the probe's recorder
    two: bool = False  # a case of the plain engine only (two tells in one case)
    id: int = -1


def msg(tag, arg=0):
    return (tag << 24) | (arg & 0xFFFFFF)


def probes():
    W = (H(0x12345678, 0x9ABCDEF0), H(0x0FEDCBA9, 0x87654321))
    out = []
    for si, (name, _, _) in enumerate(SRCS):
        senders = {"sender": (("none", NO_SENDER), ("host", N + 5), ("actor", 7))}.get(name, (("", NO_SENDER),))
        for sn, s in senders:
            out.append(Probe(f"operand/{name}{'_' + sn if sn else ''}", "opnd", *W,
                             [(s, msg(1 + si * 8 + ki, 0xABC000 + ki)) for ki in range(len(KS))]))
    pays = [0, 0x00FFFFFF, 0x01000000, 0x80000000, 0xFFFFFFFF]
    out.append(Probe("operand/payloads", "pay", *W, [(REC, p) for p in pays]))
    out.append(Probe("operand/payloads_reversed", "pay", *W, [(REC, p) for p in pays[::-1]]))
    for pi, (name, a, b) in enumerate(ORIENTED):
        out.append(Probe(f"compare/word_word/{name}", "cmpww", a, b, [(REC, msg(c, pi)) for c in range(1, 7)]))
        out.append(Probe(f"compare/word_word_tests_swapped/{name}", "cmpww_r", a, b, [(REC, msg(c, pi)) for c in (1, 2, 3, 4, 5, 6, 0)]))
        out.append(Probe(f"compare/word_const/{name}", "cmpwc", a, W[1], [(REC, msg(1 + pi * 6 + c - 1, pi)) for c in range(1, 7)]))
    for name, p, w in (("s31", 0x7FFFFFFF, 0x80000000), ("s31_rev", 0x80000000, 0x7FFFFFFF), ("s32", 0xFFFFFFFF, 1 << 32),
                       ("eq", 0xFFFFFFFF, 0xFFFFFFFF), ("lo_eq", 7, H(1, 7)), ("cross", 9, H(1, 3)), ("0_max", 0, M64),
                       ("max_0", 0xFFFFFFFF, 0)):
        out.append(Probe(f"compare/payload_word/{name}", "cmppw", w, SEL + 1, [(NO_SENDER, p)] * 7))
    for sname, (a, b) in ACT_STATES.items():
        for j, (name, *_r) in ACT_FX.items():
            out.append(Probe(f"action/{name}/{sname}", "act", a, b, [(REC, msg(j, 0x00F00D + j))] * 2))
    out.append(Probe("action/no_such_tag", "act", *W, [(REC, msg(99, 1))]))
    out.append(Probe("first_match/overlap", "fm", *W, [(REC, msg(0, a)) for a in (12, 7, 1, 7, 12)]))
    out.append(Probe("first_match/no_case", "nomatch", *W, [(REC, msg(0, a)) for a in (1, 99, 2)]))
    out.append(Probe("first_match/zero_cases", "empty", *W, [(REC, msg(1, 1)), (NO_SENDER, 0)]))
    out.append(Probe("first_match/unhandled_with_actions", "unh_act", *W, [(REC, msg(t, 3)) for t in (9, 1, 9)]))
    out.append(Probe("result/stopped_with_actions", "stop_act", *W,
                     [(REC, msg(t, a)) for t, a in ((1, 5), (2, 77), (1, 6), (1, 7), (1, 8), (2, 9))]))
    out.append(Probe("result/stopped_first", "stop_act", *W, [(REC, msg(t, a)) for t, a in ((2, 1), (1, 6), (2, 7), (1, 8), (1, 9))]))
    chain = [(REC, msg(t, a)) for t, a in ((1, 0), (1, 0), (1, 0), (0, 5), (1, 0), (0, 6), (1, 0), (0, 9), (1, 0), (0, 7), (0, 8))]
    out.append(Probe("result/become_chain", "chainA", *W, chain))
    out.append(Probe("result/become_chain_from_B", "chainB", *W, chain[1:]))
    out.append(Probe("result/become_itself", "selfbecome", *W, [(REC, msg(t, 4)) for t in (1, 0, 1, 1, 0)]))
    out.append(Probe("result/kind_past_the_tables", "badkind", *W, [(REC, msg(1, 1)), (REC, 5)]))
    for name, w in (("n", N), ("no_sender", 0xFFFFFFFF), ("2p32", 1 << 32), ("2p63", 1 << 63), ("recorder", REC),
                    ("2p32_plus_recorder", "REC+2p32")):
        out.append(Probe(f"tell/word_destination/{name}", "wdst", w, W[1], [(NO_SENDER, msg(3, 0x111)), (NO_SENDER, msg(4, 0x222))]))
    out.append(Probe("tell/sender_destination", "sdst", *W,
                     [(NO_SENDER, msg(0, 1)), (REC, msg(0, 2)), (N + 5, msg(0, 3)), (NO_SENDER, msg(1, 4)), ("REC-1", msg(1, 5))]))
    out.append(Probe("tell/payload_masks", "mask", H(0xABCDEF12, 0x34567890), H(0x11, 0xFF00FF00), [(REC, msg(t)) for t in (1, 2, 3, 4)]))
    out.append(Probe("tell/two_in_order", "two", *W, [(REC, msg(0, 0x10)), (REC, msg(1, 0)), (REC, msg(0, 0x20))], two=True))
    assert len(out) <= P, len(out)
    for i, p in enumerate(out):
        p.id = HEAD + i
    for i, s in enumerate(S_IDS):
        out.append(Probe(f"tell/self_dk/id_{s}", "selfdk", H(0x51 + i, 0x1000), H(0x61 + i, 0x2000),
                         [(NO_SENDER, msg(j, 100 * (i + 1) + j)) for j in range(1, len(DKS) + 1)], id=s))
    return out


CASES = tuple(p.name for p in probes())


def case_of(a):
    """the named case an actor belongs to: the probe itself or its recorder"""
    by_id = {p.id: p.name for p in probes()}
    return by_id.get(a, by_id.get(a - R, "sink") if HEAD + R <= a < HOLE0 else "sink")


@dataclasses.dataclass
class Program:
    single: bool
    tables: object
    probes: list
    kind: list      # per id: the registered kind (0: not registered)
    words: list     # per id: (w0, w1)
    scripts: dict   # id -> [(sender, payload)]
    commutative: frozenset  # the kinds that record commutatively

    def kind_of(self, name):
        return self.tables.kind_of(behaviors()[name])

    def with_host_tags_up_to(self, limit):
        """the program for an engine that refuses host tells of a reserved message tag (agx_stage_tells on an engine
        with timers: 0xFF): a host payload above the limit carries the limit as its tag instead"""
        cut = lambda p: p if p >> 24 <= limit else (limit << 24) | (p & 0xFFFFFF)
        return dataclasses.replace(self, scripts={a: [(s, cut(p)) for s, p in sc] for a, sc in self.scripts.items()})


@functools.lru_cache(maxsize=None)
def program(single: bool = False) -> Program:
    """the whole program, or its single-tell part (the engines with max_emit 1)"""
    bs = behaviors()
    ps = [p for p in probes() if not (single and p.two)]
    roots = [bs[n] for n in bs if not (single and n == "two")]
    tables = typed.compile_behaviors(roots, max_emit=1 if single else 2)
    assert tables.max_tells == (1 if single else 2)
    k_rec, k_sink = tables.kind_of(bs["recorder"]), tables.kind_of(bs["sink"])
    kind, words = [k_sink] * N, [None] * N
    for a in range(N):
        words[a] = (H(0x5A0000 + a, 0x00C0FFEE), H(0xDEAD, a + 1))
    for a in range(HEAD + R, HOLE0):
        kind[a] = k_rec
    for a in range(HOLE0, HOLE0 + HOLE_N):
        kind[a], words[a] = 0, (0, 0)
    scripts = {}

    def res(v, p):
        return {REC: p.id + R, "REC+2p32": p.id + R + (1 << 32), "REC-1": p.id + R - 1}.get(v, v) if isinstance(v, str) else v
    for p in ps:
        kind[p.id] = typed.KIND_COMPILED + tables.n_behaviors + 1 if p.beh == "badkind" else tables.kind_of(bs[p.beh])
        words[p.id] = (res(p.w0, p), res(p.w1, p))
        scripts[p.id] = [(res(s, p), pay) for s, pay in p.script]
    return Program(single, tables, ps, kind, words, scripts, frozenset((k_sink, tables.kind_of(bs["selfdk"]))))


def tells(prog):
    dst, src, pay = [], [], []
    for a in sorted(prog.scripts):
        for s, p in prog.scripts[a]:
            dst.append(a), src.append(s), pay.append(p)
    return np.asarray(dst, np.uint32), np.asarray(src, np.uint32), np.asarray(pay, np.uint32)


def ranges(prog, n_words=2):
    """register_range calls: runs of one kind, every actor's words (a third word carries a value of its own)"""
    out, a = [], 0
    while a < N:
        b = a
        while b < N and prog.kind[b] == prog.kind[a]:
            b += 1
        if prog.kind[a]:
            rows = np.zeros((b - a, n_words), np.uint64)
            for i in range(a, b):
                rows[i - a, 0], rows[i - a, 1] = prog.words[i]
                for x in range(2, n_words):
                    rows[i - a, x] = third_word(i, x)
            out.append((a, b - a, prog.kind[a], rows))
        a = b
    return out


def third_word(a, x=2):
    return ((0xA5 + x) << 56) | (a << 32) | (0xFFFF0000 + a)


BOUNDED_CLASS, BOUNDED_CAPACITY = 1, 4


def bounded_ids(prog):
    """the probes bound to the bounded mailbox class: the become chains (eleven and ten staged tells against four places)"""
    return [p.id for p in prog.probes if p.beh in ("chainA", "chainB")]


def workload(prog, throughput=3, n_words=2, bucket_actors=0, bounded=False, **features):
    w = wl.Workload("compiled_core", N, n_words, 1 if prog.single else 2, throughput, 0, ranges(prog, n_words),
                    behaviors=prog.tables, tells=tells(prog), bucket_actors=bucket_actors)
    if bounded:
        ids = bounded_ids(prog)
        assert ids == list(range(ids[0], ids[0] + len(ids)))
        w = dataclasses.replace(w, mailbox_classes={BOUNDED_CLASS: BOUNDED_CAPACITY}, mailboxes=[(ids[0], len(ids), BOUNDED_CLASS)])
    return dataclasses.replace(w, **features) if features else w


# ------------------------------------------------------------------ the population on the core model
COUNTERS = ("delivered", "dead_letters", "unhandled", "emitted", "staged")


def run_core(prog, ev=None, bounded=False, strict=True, own_tags=frozenset()):
    """The program on a per-message evaluator: every actor folds its host script (all of it is staged before the first
    superstep, so it is handled before anything that arrives), then what the others sent it, in the canonical order
    (sender id, emission index).  `strict`: a destination with more than one sender records commutatively and nothing
    sent in the second round sends again -- true of the rule itself, not of every mutant of it.
    Returns dict(words, alive, kinds, counts, reserved): reserved = the ids that were sent a payload whose tag is one of
    `own_tags`, the message tags a feature engine keeps for itself (such an engine handles the envelope itself, so the
    receiver ends elsewhere than the rule says; the sender does not), and whatever those ids then send to."""
    ev = ev or core.Evaluator()
    t, n = prog.tables, N
    kind, alive = list(prog.kind), [k != 0 for k in prog.kind]
    words = [list(w) for w in prog.words]
    c = dict.fromkeys(COUNTERS, 0)
    reserved = set()
    cut = {a: BOUNDED_CAPACITY for a in bounded_ids(prog)} if bounded else {}
    arrivals = {}

    def run(a, script, second):
        (kind[a], words[a][0], words[a][1], alive[a]), out, cc = ev.fold(t, n, kind[a], words[a][0], words[a][1], a, script,
                                                                         alive[a])
        c["delivered"] += cc["delivered"]
        c["unhandled"] += cc["unhandled"]
        c["dead_letters"] += cc["dead"]
        c["emitted"] += len(out)
        if any(p >> 24 in own_tags for _, p in script):
            reserved.add(a)
        for i, (d, p) in enumerate(out):
            if a in reserved or p >> 24 in own_tags:
                reserved.add(d)
            if second:
                assert not strict, f"actor {a} sends in the second round"
                c["dead_letters"] += 1
            elif d >= n or prog.kind[d] == 0:
                c["dead_letters"] += 1
            else:
                arrivals.setdefault(d, []).append((a, i, p))

    for a in sorted(prog.scripts):
        s = prog.scripts[a]
        c["staged"] += len(s)
        keep = cut.get(a, len(s))
        c["dead_letters"] += max(len(s) - keep, 0)
        run(a, s[:keep], False)
    for d in sorted(arrivals):
        q = sorted(arrivals[d])
        if strict and len({s for s, _, _ in q}) > 1:
            assert prog.kind[d] in prog.commutative, f"actor {d} has several senders and records in order"
        run(d, [(s, p) for s, _, p in q], True)
    return dict(words=[tuple(w) for w in words], alive=[int(x) for x in alive], kinds=kind, counts=c,
                reserved=sorted(x for x in reserved if x < n))


def census(prog):
    """what the program exercises on the core model (a Census)"""
    total = core.Census()
    run_core(prog, core.Evaluator(total))
    return total


# ------------------------------------------------------------------ the feature variants
@dataclasses.dataclass(frozen=True)
class Variant:
    """One feature engine with the feature switched on and not used."""
    features: dict          # the Workload fields that switch it on
    model: str              # "module:Class" of the feature's model under tests/
    infos: dict             # info call -> the keys that stay 0 while the feature never fires
    copy: str               # the compiled_apply copy of akka_amd/csrc/agx_device.h such an engine runs
    witness: tuple          # (method, arguments, text): a call that only an engine of this variant answers with an
                            # AgxError holding `text` (text None: only such an engine answers at all); on an engine
                            # without the feature the call succeeds or is refused in other words
    own_tags: frozenset = frozenset()  # the message tags the engine keeps for itself
    host_tag_limit: int = 0xFF         # the largest tag a host tell may carry (agx_stage_tells refuses the engine's own)


def variants(prog):
    """name -> Variant.  The entity range and the child block are the four ids nobody registers; the supervisor entries
    stand on the sinks' behaviour, which never fails."""
    k_sink, nb = prog.kind_of("sink"), prog.tables.n_behaviors
    on_sink = lambda row: [row if typed.KIND_COMPILED + i == k_sink else [] for i in range(nb)]
    resume = on_sink([typed.AgxSupervisor(class_mask=0xFFFFFFFF, strategy=typed.SUP_RESUME)])
    restart = on_sink([typed.AgxSupervisor(class_mask=0xFFFFFFFF, strategy=typed.SUP_RESTART, max_restarts=-1, within=1)])
    backoff = on_sink([typed.AgxBackoff(1, 2, 0, 1, -1)])
    entity = [(HOLE0, HOLE_N, k_sink, 0, 0, msg(0x0F, 1), 0, 0)]
    recep = {"n_keys": 1, "capacity": 8}
    # ("discarded" is left out: an envelope of tag 0xFF / 0xFB that a probe sends counts there as a stale timer or
    # receive-timeout message, which is not the feature firing; "late" of an ask likewise counts tells to ids >= 2^31)
    timer_keys, ask_keys, rt_keys = ("fired", "active", "pending"), ("asked", "answered", "timed_out"), ("fired", "set", "pending")
    recep_keys = ("routed", "no_routees", "registered", "deregistered")
    sup_keys = ("failures", "resumes", "restarts")
    TM, RT = frozenset({0xFF}), frozenset({0xFF, 0xFB})
    return {
        "stash": Variant(dict(mailbox_classes={1: 0}, mailboxes=[(HEAD, P, 1)], stash={1: 4}), "stash_model:StashModel",
                         {"stash_info": ("stashed", "unstashed", "overflows", "held", "pending")}, "compiled_apply<kStash>",
                         ("set_timers", (1,), "without a deque-based mailbox class (agx_set_stash)")),
        "priority": Variant(dict(mailbox_priorities={0: bytes(256)}), "prio_model:PrioModel", {}, "compiled_apply",
                            ("set_timers", (1,), "without priority tables (agx_set_mailbox_priority)")),
        "timers": Variant(dict(timers={"n_keys": 1}), "timer_model:TimerModel", {"timer_info": timer_keys}, "compiled_apply_tm",
                          ("set_death_watch", (1,), "without timers (agx_set_timers)"), TM, 0xFA),
        "receive_timeout": Variant(dict(timers={"n_keys": 1, "receive_timeout": {"transparent": ()}}),
                                   "receive_timeout_model:ReceiveTimeoutModel",
                                   {"timer_info": timer_keys, "receive_timeout_info": rt_keys}, "compiled_apply_tm<kIdle>",
                                   ("set_ask", (), "without receive timeouts (agx_set_receive_timeout)"), RT, 0xFA),
        "ask": Variant(dict(timers={"n_keys": 1, "ask": True}), "ask_model:AskModel",
                       {"timer_info": timer_keys, "ask_info": ask_keys}, "compiled_apply_tm<kAsk>",
                       ("set_receive_timeout", ((),), "without the ask pattern (agx_set_ask)"), TM, 0xFA),
        "sharding": Variant(dict(timers={"n_keys": 1, "receive_timeout": {"transparent": (), "sharding": entity}}),
                            "sharding_model:ShardingModel",
                            {"timer_info": timer_keys, "receive_timeout_info": rt_keys,
                             "sharding_info": ("started", "restarted", "passivations", "passivated", "passivate_ignored",
                                               "passivate_unknown", "alive")}, "compiled_apply_tm<kIdle, kShard>",
                            ("set_sharding", (entity,), "sharding is set already"), RT, 0xFA),
        "watch": Variant(dict(watch={"n_slots": 1}), "watch_model:WatchModel",
                         {"watch_info": ("watches", "terminated", "discarded", "death_pacts", "conflicts", "watching", "pending")},
                         "compiled_apply_w", ("set_timers", (1,), "without death watch (agx_set_death_watch)"), frozenset({0xFE})),
        "children": Variant(dict(watch={"n_slots": 1}, children={"regions": [(1, 1, HOLE0, HOLE_N)], "sites": [(k_sink, 0, 0)]}),
                            "children_model:ChildrenModel",
                            {"children_info": ("spawned", "refused", "created", "child_stops", "cascade_stops", "illegal_stops", "live")},
                            "compiled_apply_c", ("spawn_children", (1, 0, 99), "spawn site 99 of 1"), frozenset({0xFE, 0xFD, 0xFC})),
        "supervision": Variant(dict(supervision={"rows": resume}), "supervision_model:SupervisionModel",
                               {"supervision_info": sup_keys}, "compiled_apply_s",
                               ("set_timers", (1,), "without supervision (agx_set_supervision)")),
        "backoff": Variant(dict(supervision={"rows": restart, "backoff": backoff}), "backoff_model:BackoffModel",
                           {"supervision_info": sup_keys,
                            "backoff_info": ("backoffs", "resumed", "dropped", "limit_stops", "suspended")},
                           "compiled_apply_s (backoff)", ("set_backoff", (backoff,), "backoff is set once")),
        "receptionist": Variant(dict(receptionist=recep), "receptionist_model:ReceptionistModel", {"receptionist_info": recep_keys},
                                "compiled_apply_rc", ("set_timers", (1,), "without the receptionist (agx_set_receptionist)")),
        "topics": Variant(dict(receptionist=recep, topics={"log_capacity": 16}), "topic_model:TopicModel",
                          {"receptionist_info": recep_keys,
                           "topic_info": ("published", "fanned_out", "no_subscribers", "host_published")}, "compiled_apply_tp",
                          ("set_router_logics", (0, 0, 0), "without topics (agx_set_topics)")),
        "listings": Variant(dict(receptionist=recep, topics={"log_capacity": 16}, listings={"payloads": [0]}),
                            "listing_model:ListingModel",
                            {"receptionist_info": recep_keys, "listing_info": ("subscribes", "finds", "listings_sent", "notified")},
                            "compiled_apply_ls", ("listing_info", (), None)),
        "router_logics": Variant(dict(receptionist=recep, router_logics={"hashed_keys_mask": 0, "virtual_nodes_factor": 0, "seed": 7}),
                                 "router_model:RouterModel", {"receptionist_info": recep_keys, "router_info": ("hashed", "random")},
                                 "compiled_apply_hr", ("set_topics", (16,), "without router logics (agx_set_router_logics)")),
    }


VARIANT_NAMES = ("stash", "priority", "timers", "receive_timeout", "ask", "sharding", "watch", "children", "supervision",
                 "backoff", "receptionist", "topics", "listings", "router_logics")


def witness_text(engine, witness):
    """what the engine answers to a variant's witness call: the refusal's text, or None when it answers"""
    from akka_amd._lib import AgxError
    method, args, _ = witness
    try:
        getattr(engine, method)(*args)
    except AgxError as e:
        return str(e)
    return None


def is_variant(engine, witness):
    text = witness_text(engine, witness)
    return text is None if witness[2] is None else text is not None and witness[2] in text


def model_of(spec):
    import importlib
    mod, cls = spec.split(":")
    return getattr(importlib.import_module(f"tests.{mod}"), cls)


def variant_snapshot(target, infos):
    """after the run: state words, alive flags, kinds and the feature's info"""
    words, alive = target.read_state()
    kinds = target.read_kinds() if hasattr(target, "read_kinds") else target.kind.astype(np.uint8)
    return words, alive & 1, np.asarray(kinds, np.uint8), {i: dict(getattr(target, i)()) for i in infos}
