"""The conformance program of the compiled-behaviour rule, without a GPU (DESIGN.md §8 "The compiled rule at 64-bit
edges"): the three references agree on it, it exercises what it claims to, and it tells every mutant of the rule from
the rule."""
import functools

import numpy as np
import pytest

from akka_amd import typed
from tests import compiled_core_cases as C
from tests import compiled_core_model as core
from tests.prio_model import PrioModel

M64, M32 = core.M64, core.M32
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")


def on_target(target, w):
    w.apply_to(target)
    st = target.run()
    words, alive = target.read_state()
    kinds = target.read_kinds() if hasattr(target, "read_kinds") else target.kind.astype(np.uint8)
    target.close()
    return dict(st), words, alive, np.asarray(kinds, np.uint8)


@functools.lru_cache(maxsize=None)
def references(single, throughput, bounded=False):
    from oracle import BspOracle
    prog = C.program(single)
    w = C.workload(prog, throughput, bounded=bounded)
    return (prog, on_target(BspOracle(**w.engine_kwargs()), w), on_target(PrioModel(**w.engine_kwargs()), w),
            C.run_core(prog, bounded=bounded))


def assert_core(core_run, st, words, alive, kinds, name, skip=()):
    """the core model's fold against a population run: every state word, alive flag, kind and counter it knows"""
    for k in core_run["counts"]:
        assert core_run["counts"][k] == st[k], f"{name}: {k} core={core_run['counts'][k]} run={st[k]}"
    for a in range(C.N):
        if a in skip:
            continue
        got = (int(words[a, 0]), int(words[a, 1]), int(alive[a]) & 1, int(kinds[a]))
        want = (*core_run["words"][a], core_run["alive"][a], core_run["kinds"][a])
        assert got == want, f"{name}: actor {a}: run {[hex(x) for x in got]} core {[hex(x) for x in want]}"


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("throughput", [1, 3])
@pytest.mark.parametrize("single", [False, True])
def test_three_references_agree(single, throughput, bounded):
    prog, (so, wo, ao, ko), (sm, wm, am, km), cr = references(single, throughput, bounded)
    for k in COUNT_KEYS:
        assert so[k] == sm[k], (k, so[k], sm[k])
    assert so["in_flight"] == 0 and so["staged"] + so["emitted"] == so["delivered"] + so["dead_letters"]
    assert np.array_equal(wo, wm) and np.array_equal(ao, am) and np.array_equal(ko, km)
    assert_core(cr, so, wo, ao, ko, "oracle")
    assert_core(cr, sm, wm, am, km, "model")


@pytest.mark.parametrize("single", [False, True])
def test_census(single):
    """the program runs what it claims to: the single-tell part (the feature engines') no less than the whole"""
    prog = C.program(single)
    cen = C.census(prog)
    for op in (core.A_SET, core.A_ADD, core.A_MAX, core.A_MIN):
        for word in (0, 1):
            assert (op, word) in cen.ops, (op, word)
    assert (core.A_TELL, 0) in cen.ops
    for cmp in range(1, 7):
        for outcome in (True, False):
            assert (cmp, outcome) in cen.cmps, (cmp, outcome)
    assert cen.results == {core.SAME, core.STOPPED, core.UNHANDLED, core.BECOME}
    assert {(True, False), (False, None), (True, True)} <= cen.first_second
    taken = set(cen.cases)
    never = [ci for ci in range(int(prog.tables.first[-1])) if ci not in taken]
    # (a case nobody takes is a comparison that is false for its pair: it was tried, and it has two tests)
    lazy = [ci for ci in never if typed.CMP_ANY in (prog.tables.cases[ci].cmp1, prog.tables.cases[ci].cmp2)]
    assert not lazy, f"cases no message takes: {lazy}"
    r = C.run_core(prog)
    assert r["counts"]["dead_letters"] > 0 and r["counts"]["unhandled"] > 0
    assert any(w >= 1 << 63 for ws in r["words"] for w in ws)
    assert any(w and not w & M32 for ws in r["words"] for w in ws), "no word ends with a zero low half under a high half"
    assert any(k != k0 for k, k0 in zip(r["kinds"], prog.kind)), "no become stands at the end"
    # a become followed by a message in the same drain window (throughput 3: the messages 3i .. 3i + 2 of a script)
    t, hit = prog.tables, False
    for p in prog.probes:
        kind, w0, w1 = prog.kind[p.id], *prog.words[p.id]
        for i, (s, pay) in enumerate(prog.scripts[p.id]):
            kind, w0, w1, res, _ = core.step(t, C.N, kind, w0, w1, p.id, s, pay)
            hit |= res == core.BECOME and i % 3 != 2 and i + 1 < len(prog.scripts[p.id])
    assert hit
    # every source with every k, every payload and sender the cases name
    acts = [t.acts[i] for i in range(t.n_acts)]
    for _, src, word in C.SRCS:
        for k in C.KS:
            assert any(a.src == src and a.sword == word and a.k == k for a in acts), (src, word, k)
    pays = {p for s in prog.scripts.values() for _, p in s}
    assert {0, 0x00FFFFFF, 0x01000000, 0x80000000, 0xFFFFFFFF} <= pays
    senders = {s for sc in prog.scripts.values() for s, _ in sc}
    assert C.NO_SENDER in senders and any(C.N <= s < C.NO_SENDER for s in senders)
    assert {a.dk for a in acts if a.op == core.A_TELL and a.dsrc == core.V_SELF} >= set(C.DKS)
    assert all(any(p.id == s and p.beh == "selfdk" for p in prog.probes) for s in (0, C.N - 1))
    assert (t.max_tells == 2) != single


# ------------------------------------------------------------------ the mutants
class SignedCompare(core.Evaluator):
    def compare(self, op, a, b):
        s = lambda x: x - (1 << 64) if x >> 63 else x
        return super().compare(op, s(a), s(b))


class Add32(core.Evaluator):
    def add(self, a, b):
        return (a & ~M32) | ((a + b) & M32)


class MaxMinSwapped(core.Evaluator):
    def maximum(self, a, b):
        return min(a, b)

    def minimum(self, a, b):
        return max(a, b)


class CompareLowHalf(core.Evaluator):
    def compare(self, op, a, b):
        return super().compare(op, a & M32, b & M32)


class WordFlipped(core.Evaluator):
    def word_index(self, word):
        return (word ^ 1) & 1


class WordAlwaysZero(core.Evaluator):
    """(an index that is not masked cannot be told from the rule on tables agx_set_behaviors accepts -- it refuses a
    word above 1 -- so the wrong masks are this one and the flip)"""

    def word_index(self, word):
        return 0


class ActionsReadOldState(core.Evaluator):
    def action_view(self, before, now):
        return list(before)


class LastMatch(core.Evaluator):
    def pick(self, matching):
        return matching[-1]


class BecomeOneLate(core.Evaluator):
    def fold(self, tables, n, kind, w0, w1, self_id, script, alive=True):
        self._pending = None
        return super().fold(tables, n, kind, w0, w1, self_id, script, alive)

    def step(self, tables, n, kind, w0, w1, self_id, sender, payload):
        nxt, self._pending = getattr(self, "_pending", None), None
        k, w0, w1, res, sent = super().step(tables, n, kind, w0, w1, self_id, sender, payload)
        if k != kind:
            self._pending, k = k, kind
        if nxt is not None and self._pending is None:
            k = nxt
        return k, w0, w1, res, sent


class CRemainder(core.Evaluator):
    def self_destination(self, self_id, dk, n):
        x = self_id + dk
        r = abs(x) % n
        return (-r if x < 0 else r) & M64


class SelfPlusDk32(core.Evaluator):
    def self_destination(self, self_id, dk, n):
        x = (self_id + dk) & M32
        x = x - (1 << 32) if x >> 31 else x
        return x % n


class DestinationTruncated(core.Evaluator):
    def clamp_destination(self, d):
        return d & M32


class OrMaskWithoutCut(core.Evaluator):
    def tell_payload(self, v, or_mask):
        return ((v | or_mask) & M32) if or_mask else (v & M32)


class AlwaysCutTo24(core.Evaluator):
    def tell_payload(self, v, or_mask):
        return (v & 0xFFFFFF) | or_mask


MUTANTS = {m.__name__: m for m in (SignedCompare, Add32, MaxMinSwapped, CompareLowHalf, WordFlipped, WordAlwaysZero,
                                   ActionsReadOldState, LastMatch, BecomeOneLate, CRemainder, SelfPlusDk32,
                                   DestinationTruncated, OrMaskWithoutCut, AlwaysCutTo24)}


def killers(prog, mutant):
    """the named cases whose probe, recorder or counters a mutant changes"""
    true, got = C.run_core(prog), C.run_core(prog, mutant(), strict=False)
    names = []
    for p in prog.probes:
        # (a V_SELF probe's envelopes go to the sinks and to the V_SELF probes around it)
        ids = [a for a in range(C.N) if prog.kind[a] in prog.commutative] if p.beh == "selfdk" else (p.id, p.id + C.R)
        if any((true[k][a] != got[k][a]) for a in ids for k in ("words", "alive", "kinds")):
            names.append(p.name)
    return names, true["counts"] != got["counts"]


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("name", list(MUTANTS))
def test_program_kills_mutant(name, single):
    """a rule that is wrong in one clause ends the program elsewhere than the rule: in the state of a probe or of its
    recorder (the counters alone would do, but the GPU tests report states first)"""
    names, counts = killers(C.program(single), MUTANTS[name])
    assert names, f"{name} survives (counters differ: {counts})"


def test_the_true_evaluator_is_no_mutant():
    prog = C.program()
    assert killers(prog, core.Evaluator) == ([], False)


def test_tag_zero_message_type_is_not_cut():
    """include/akka_gpu.h AGX_A_TELL: the 24-bit cut comes with a message tag, or_mask != 0.  A MessageType of tag 0
    lowers to or_mask 0, so its argument goes out as the low 32 bits, uncut."""
    prog = C.program()
    p = next(p for p in prog.probes if p.name == "tell/payload_masks")
    _, out, _ = core.fold(prog.tables, C.N, prog.kind[p.id], *prog.words[p.id], p.id, prog.scripts[p.id])
    w0, w1 = prog.words[p.id]
    assert [pay for _, pay in out] == [(w0 & 0xFFFFFF) | 0x55000000, w0 & M32, w0 & M32, (w1 & 0xFFFFFF) | 1]
    assert all(d == p.id + C.R for d, _ in out)


def test_step_known_answers():
    """a few lines of the ABI text by hand"""
    mk = lambda **k: typed.AgxCase(**k)
    cases = (typed.AgxCase * 2)(mk(src1=core.V_WORD, word1=0, cmp1=core.CMP_LT, src2=core.V_WORD, word2=1, result=core.BECOME,
                                   next=0, act_first=0, act_count=3), mk(result=core.STOPPED, act_first=3, act_count=1))
    acts = (typed.AgxAct * 4)(typed.AgxAct(op=core.A_ADD, word=0, src=core.V_CONST, k=-1),
                              typed.AgxAct(op=core.A_MAX, word=1, src=core.V_WORD, sword=0),
                              typed.AgxAct(op=core.A_TELL, src=core.V_WORD, sword=1, dsrc=core.V_SELF, dk=-3),
                              typed.AgxAct(op=core.A_TELL, src=core.V_PAYLOAD, k=1, dsrc=core.V_SENDER, dk=1, or_mask=0x7F000000))
    t = typed.Tables([typed.Behavior("b", typed.State())], cases, acts, np.asarray([0, 2], np.uint32), 4)
    # 0 < 2^63: 0 - 1 wraps to 2^64 - 1, the max takes it, the tell goes to (1 - 3) mod 10 = 8 with the low 32 bits
    assert core.step(t, 10, 16, 0, 1 << 63, 1, 5, 9) == (16, M64, M64, core.BECOME, [(8, M32)])
    # 2^63 < 1 is false unsigned: the second case; sender 2^32 - 1 + 1 is clamped, the payload is cut and tagged
    assert core.step(t, 10, 16, 1 << 63, 1, 1, M32, 0x12FFFFFF) == (16, 1 << 63, 1, core.STOPPED, [(M32, 0x7F000000)])
    assert core.step(t, 10, 17, 3, 4, 1, 5, 9) == (17, 3, 4, core.UNHANDLED, [])


@pytest.mark.parametrize("variant", C.VARIANT_NAMES)
def test_feature_models_agree_with_the_fold(variant):
    """the single-tell part with a feature switched on and not used: the feature's model ends where the core model's
    fold ends (but for the actors that are sent a message tag such an engine keeps for itself), and the feature never
    fires"""
    prog = C.program(True)
    v = C.variants(prog)[variant]
    prog = prog.with_host_tags_up_to(v.host_tag_limit)
    w = C.workload(prog, 3, bucket_actors=32, **v.features)
    m = C.model_of(v.model)(**w.engine_kwargs())
    w.apply_to(m)
    st = dict(m.run())
    words, alive, kinds, info = C.variant_snapshot(m, v.infos)
    cr = C.run_core(prog, own_tags=v.own_tags)
    for i, keys in v.infos.items():
        assert all(info[i][k] == 0 for k in keys), (i, info[i])
    assert st["in_flight"] == 0 and st["staged"] == cr["counts"]["staged"]
    skip = set(cr["reserved"])
    assert bool(skip) == (0xFF in v.own_tags), (variant, sorted(skip))  # (the probes send 0xFF.., no other such tag)
    assert len(skip) < C.N // 8
    # (with such envelopes the engine's counters differ from the rule's as well: the states of the others still hold)
    assert_core(dict(cr, counts={}) if skip else cr, st, words, alive, kinds, variant, skip)
