"""The compiled-behaviour rule (include/akka_gpu.h "compiled behaviours") as one per-message evaluator over Python
ints, written from the ABI text and from nothing else: no numpy integer arithmetic, nothing from the feature models.

  * an operand is base(src, word) + k mod 2^64, base = 0, the payload, its tag (payload >> 24), its argument
    (payload & 0xFFFFFF), state word `word`, the sender id or the actor's own id;
  * the six comparisons are unsigned 64-bit, AGX_CMP_ANY holds always;
  * the cases of behaviour kind - AGX_KIND_COMPILED are tried in order and the first whose two tests hold is taken; no
    case, or a kind that names no behaviour of the tables, is Behaviors.unhandled with the state untouched;
  * its actions run in order, and each reads the words as the earlier ones left them: set, add (wrapping), max and min
    (unsigned) on words 0 and 1, and tell;
  * a tell's destination is (self + dk) mod n for a destination based on the actor's own id, otherwise the destination
    operand clamped to 0xFFFFFFFF; its payload is (v & 0xFFFFFF) | or_mask with a message tag (or_mask != 0), else the
    low 32 bits of v;
  * the result is same, stopped, unhandled or become; a become changes the kind the next message meets.

`Evaluator` keeps every clause in a method of its own, so a test can swap one clause for a wrong one (the mutants of
tests/test_compiled_core_model.py) and ask whether the conformance program notices.  `step` and `fold` are the true
rule."""
from __future__ import annotations

M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
KIND_COMPILED = 16
V_CONST, V_PAYLOAD, V_TAG, V_ARG, V_WORD, V_SENDER, V_SELF = range(7)
CMP_ANY, CMP_EQ, CMP_NE, CMP_LT, CMP_LE, CMP_GT, CMP_GE = range(7)
A_SET, A_ADD, A_MAX, A_MIN, A_TELL = 1, 2, 3, 4, 5
SAME, STOPPED, UNHANDLED, BECOME = 0, 1, 2, 3


class Census:
    """what a run of the evaluator has exercised"""

    def __init__(self):
        self.ops = set()        # (action op, word)
        self.cmps = set()       # (cmp, outcome)
        self.results = set()    # result codes taken (UNHANDLED also for "no case")
        self.first_second = set()  # (test 1 held, test 2 held) of the cases tried (test 2 only when test 1 held)
        self.cases = {}         # case index -> times taken

    def merge(self, o: "Census"):
        self.ops |= o.ops
        self.cmps |= o.cmps
        self.results |= o.results
        self.first_second |= o.first_second
        for k, v in o.cases.items():
            self.cases[k] = self.cases.get(k, 0) + v


class Evaluator:
    def __init__(self, census: Census | None = None):
        self.census = census

    # ---- the clauses
    def word_index(self, word: int) -> int:
        return word & 1

    def base(self, src, word, w, sender, self_id, payload) -> int:
        if src == V_PAYLOAD:
            return payload
        if src == V_TAG:
            return payload >> 24
        if src == V_ARG:
            return payload & 0xFFFFFF
        if src == V_WORD:
            return w[self.word_index(word)]
        if src == V_SENDER:
            return sender
        if src == V_SELF:
            return self_id
        return 0

    def operand(self, src, word, k, w, sender, self_id, payload) -> int:
        return (self.base(src, word, w, sender, self_id, payload) + k) & M64

    def compare(self, op, a, b) -> bool:
        if op == CMP_EQ:
            return a == b
        if op == CMP_NE:
            return a != b
        if op == CMP_LT:
            return a < b
        if op == CMP_LE:
            return a <= b
        if op == CMP_GT:
            return a > b
        if op == CMP_GE:
            return a >= b
        return True

    def add(self, a, b) -> int:
        return (a + b) & M64

    def maximum(self, a, b) -> int:
        return a if a >= b else b

    def minimum(self, a, b) -> int:
        return a if a <= b else b

    def self_destination(self, self_id, dk, n) -> int:
        return (self_id + dk) % n  # (Python's %: the mathematical residue, 0..n-1)

    def clamp_destination(self, d) -> int:
        return M32 if d > M32 else d

    def tell_payload(self, v, or_mask) -> int:
        return ((v & 0xFFFFFF) | or_mask) if or_mask else (v & M32)

    def pick(self, matching: list) -> int:
        """the case to run, of the indices of all matching cases in table order"""
        return matching[0]

    def action_view(self, w_before, w_now):
        """the words an action's operands read"""
        return w_now

    def _test(self, cmp, a, b) -> bool:
        r = self.compare(cmp, a, b)
        if self.census is not None and cmp != CMP_ANY:
            self.census.cmps.add((cmp, r))
        return r

    def matches(self, C, w, sender, self_id, payload) -> bool:
        t1 = self._test(C.cmp1, self.operand(C.src1, C.word1, C.k1, w, sender, self_id, payload),
                        self.operand(C.src2, C.word2, C.k2, w, sender, self_id, payload))
        if not t1:
            if self.census is not None:
                self.census.first_second.add((False, None))
            return False
        t2 = self._test(C.cmp2, self.operand(C.src3, C.word3, C.k3, w, sender, self_id, payload),
                        self.operand(C.src4, C.word4, C.k4, w, sender, self_id, payload))
        if self.census is not None:
            self.census.first_second.add((True, t2))
        return t2

    # ---- the rule
    def step(self, tables, n, kind, w0, w1, self_id, sender, payload):
        """one message: (kind', w0', w1', result, [(dst, payload), ...])"""
        b = kind - KIND_COMPILED
        sent = []
        if b < 0 or b >= tables.n_behaviors:
            self._result(UNHANDLED)
            return kind, w0, w1, UNHANDLED, sent
        lo, hi = int(tables.first[b]), int(tables.first[b + 1])
        w = [w0, w1]
        matching = []
        for ci in range(lo, hi):
            if self.matches(tables.cases[ci], w, sender, self_id, payload):
                matching.append(ci)
                if type(self).pick is Evaluator.pick:
                    break  # (first match: the later cases are not even tried)
        if not matching:
            self._result(UNHANDLED)
            return kind, w0, w1, UNHANDLED, sent
        ci = self.pick(matching)
        C = tables.cases[ci]
        if self.census is not None:
            self.census.cases[ci] = self.census.cases.get(ci, 0) + 1
        before = (w0, w1)
        for i in range(C.act_first, C.act_first + C.act_count):
            A = tables.acts[i]
            view = self.action_view(before, w)
            v = self.operand(A.src, A.sword, A.k, view, sender, self_id, payload)
            x = self.word_index(A.word)
            if self.census is not None:
                self.census.ops.add((A.op, x if A.op != A_TELL else 0))
            if A.op == A_SET:
                w[x] = v
            elif A.op == A_ADD:
                w[x] = self.add(w[x], v)
            elif A.op == A_MAX:
                w[x] = self.maximum(w[x], v)
            elif A.op == A_MIN:
                w[x] = self.minimum(w[x], v)
            elif A.op == A_TELL:
                if A.dsrc == V_SELF:
                    d = self.self_destination(self_id, A.dk, n)
                else:
                    d = self.operand(A.dsrc, A.dword, A.dk, view, sender, self_id, payload)
                sent.append((self.clamp_destination(d) & M32, self.tell_payload(v, A.or_mask) & M32))
        res = C.result
        self._result(res)
        if res == BECOME:
            return KIND_COMPILED + C.next, w[0], w[1], BECOME, sent
        return kind, w[0], w[1], res, sent

    def _result(self, r):
        if self.census is not None:
            self.census.results.add(r)

    def fold(self, tables, n, kind, w0, w1, self_id, script, alive=True):
        """one actor over a FIFO list of (sender, payload): the final (kind, w0, w1, alive), the envelopes it sent
        [(dst, payload), ...] in order, and its counters (delivered, unhandled, dead: the mail behind a stop)"""
        out = []
        delivered = unhandled = dead = 0
        for sender, payload in script:
            if not alive:
                dead += 1
                continue
            kind, w0, w1, res, sent = self.step(tables, n, kind, w0, w1, self_id, sender, payload)
            out += sent
            delivered += 1
            if res == UNHANDLED:
                unhandled += 1
            if res == STOPPED:
                alive = False
        return (kind, w0, w1, alive), out, dict(delivered=delivered, unhandled=unhandled, dead=dead)


_TRUE = Evaluator()


def step(tables, n, kind, w0, w1, self_id, sender, payload):
    return _TRUE.step(tables, n, kind, w0, w1, self_id, sender, payload)


def fold(tables, n, kind, w0, w1, self_id, script, alive=True):
    return _TRUE.fold(tables, n, kind, w0, w1, self_id, script, alive)
