"""The scenarios of the priority-mailbox tests, shared by the CPU file (tests/test_prio_model.py: the
model against the frozen oracle, the known answers, and the guard that no scenario is vacuous) and
the GPU file (tests/test_gpu_priority_mailboxes.py: the engine against the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "priority_mailbox_kats.json").read_text())

N_KAT, ECHO_ACTOR, RESULT_TAG = 64, 37, 255
KAT_T = (1, 5, 300)
KAT_CAPACITY = (0, 1000, 150)          # unbounded, the spec's bounded capacity, one that drops the tail


def echo_population(throughput: int, capacity: int, n: int = N_KAT) -> wl.Workload:
    """`n` echo actors (typed.echo: every message goes on, unchanged, to host id `n`) on class 0."""
    e = typed.echo(n)
    tb = typed.compile_behaviors([e], max_emit=1)
    return wl.Workload("echo", n, 2, 1, throughput, capacity, [(0, n, tb.kind_of(e), None)], behaviors=tb,
                       outbound=(n, 1), bucket_actors=32)


def stable_table() -> bytes:
    """StablePriorityDispatcherSpec's priority function over message tags: tag i (the integer i) ->
    min(i, 101), Result (tag 255) and the unused tags last."""
    p = KATS["stable_priority"]["priority"]
    assert p["int_up_to"] == 100 and p["other_int"] == 101
    return bytes(min(t, p["other_int"]) if t <= 200 else 255 for t in range(256))


def stable_kat(throughput: int, capacity: int):
    """(workload, expected echo payloads, expected dead letters): the integers 1..200 as tags, in the
    fixture's shuffled order, then Result, all to one actor before the first run."""
    sent = [int(x) for x in KATS["stable_priority"]["send_order"]] + [RESULT_TAG]
    w = echo_population(throughput, capacity)
    dst = np.full(len(sent), ECHO_ACTOR, np.uint32)
    w.tells = (dst, np.full(len(sent), NO_SENDER, np.uint32), (np.asarray(sent, np.uint32) << np.uint32(24)))
    w.mailbox_priorities = {0: stable_table()}
    adm = sent if capacity == 0 else sent[:capacity]   # offer fails on a full queue, whatever the priority
    lo = sorted(x for x in adm if x <= 100)
    hi = [x for x in adm if 100 < x <= 200]
    exp = lo + hi + [x for x in adm if x == RESULT_TAG]
    return w, np.asarray(exp, np.uint32) << np.uint32(24), len(sent) - len(adm)


CONTROL_TAGS = {"test": 1, "test2": 2, "ImportantMessage": 3}


def control_table() -> bytes:
    ctl = {CONTROL_TAGS[m] for m in KATS["control_aware"]["control"]}
    return bytes(0 if t in ctl else 1 for t in range(256))


def control_kat(capacity: int):
    k = KATS["control_aware"]
    w = echo_population(5, capacity)
    sent = [CONTROL_TAGS[m] for m in k["send_order"]]
    w.tells = (np.full(3, ECHO_ACTOR, np.uint32), np.full(3, NO_SENDER, np.uint32),
               np.asarray(sent, np.uint32) << np.uint32(24))
    w.mailbox_priorities = {0: control_table()}
    return w, np.asarray([CONTROL_TAGS[m] for m in k["expected"]], np.uint32) << np.uint32(24)


def overtake(target):
    """T = 2: six normal messages and one superstep, then two control messages: they are at the head of
    superstep 2.  `target` is an engine or the model; returns (counters, echoed payloads)."""
    w = echo_population(2, 0)
    w.mailbox_priorities = {0: control_table()}
    w.apply_to(target)
    normal = (np.uint32(1) << np.uint32(24)) | np.arange(6, dtype=np.uint32)
    target.tell(np.full(6, ECHO_ACTOR, np.uint32), normal)
    target.run(1)
    control = (np.uint32(3) << np.uint32(24)) | np.arange(2, dtype=np.uint32)
    target.tell(np.full(2, ECHO_ACTOR, np.uint32), control)
    st = target.run()
    return st, target.take_outbound()[2], normal, control


# population parity: (seed, throughput) of wl.priority_mix(2048, ...)
POPULATION = [(11, 1), (12, 3)]
POPULATION_BUCKETS = (32, 2048)

# the new path against the frozen oracle: wl.mailbox_mix(6000, ...) with a constant table on every class
CONSTANT_TC = [(1, 0), (3, 0), (5, 4), (50, 1)]
CONSTANT_BUCKET_ACTORS = 128   # (test_prio_model.py checks that no bucket's inbox exceeds one tile)
TILE = 2048


def constant_mix(T: int, C: int) -> wl.Workload:
    w = wl.mailbox_mix(6000, seed=T + C, throughput=T, capacity=C)
    w.mailbox_priorities = {c: bytes([7] * 256) for c in (0, 1, 2, 3)}
    return w


# pre-sorted equivalence: one superstep, T >= every inbox
PRESORT_SEED, PRESORT_T = 21, 64


def presorted():
    """(workload with the tables and host tells in random order, the same workload without tables and
    the tells stably pre-sorted per destination by priority)."""
    w = wl.priority_mix(2048, seed=PRESORT_SEED, throughput=PRESORT_T)
    w.mailbox_classes = {1: 0, 2: 0, 3: 0}   # unbounded: the FIFO oracle admits the same set
    ref = wl.priority_mix(2048, seed=PRESORT_SEED, throughput=PRESORT_T, tables=False)
    ref.mailbox_classes = dict(w.mailbox_classes)
    dst, src, pay = w.tells
    assert np.bincount(dst).max() <= PRESORT_T
    cls = np.zeros(w.n_actors, np.int64)
    for first, count, c in w.mailboxes:
        cls[first:first + count] = c
    key = np.zeros(dst.size, np.int64)
    for c, tab in w.mailbox_priorities.items():
        m = cls[dst] == c
        key[m] = np.frombuffer(tab, np.uint8)[pay[m] >> 24]
    o = np.argsort(key, kind="stable")       # (the inbox formation then groups by destination, stably)
    ref.tells = (dst[o], src[o], pay[o])
    return w, ref
