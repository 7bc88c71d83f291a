"""Host calls between two runs (DESIGN.md §8 "Between runs"): agx_register_range and agx_set_mailbox after a run
bring the device's actors back to the host mirror (sync_mirrors), and the next run uploads the whole mirror again
(prepare_run: kinds, flags, the state in the device's layout).  Three kinds of test walk that round trip with mail in
flight, every one bit-exact against the BSP oracle or a feature's model after every leg:

1. neutral calls -- a zero-count register_range, a zero-count set_mailbox, a re-binding of actors to the mailbox class
   they have -- before every run after the first must change nothing (counters, state words, alive flags, kinds);
2. real registrations between runs (a range unregistered with mail queued for it, part of it registered again with
   a non-zero state, ids that never were registered) over the pipelines and every device state layout;
3. reads while the mirror is the newer side, and agx_read_state of sub-ranges.

Every case first asserts on the reference side that it tests something: mail in flight at the boundary, kinds (or
alive flags) that differ from the registered ones, dead letters made by the unregistering leg."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import CRDT_WORDS, EngineConfig, GpuEngine, Kind, owner
from tests import crdt_cases as C
from tests.test_gpu_parity import COUNT_KEYS, assert_same

pytestmark = pytest.mark.gpu

PIPELINES = {
    "fused": {},
    "bits3": {"AGX_RADIX_BITS": "3"},
    "bits3_ring1": {"AGX_RADIX_BITS": "3", "AGX_RING_APPLY": "1"},
    "bits3_ring0": {"AGX_RADIX_BITS": "3", "AGX_RING_APPLY": "0"},
    "unfused": {"AGX_NO_FUSED": "1"},
}
SHARDED_KEYS = tuple(k for k in COUNT_KEYS if k != "supersteps")  # (as test_loopback_sharded)
QUIET = 1 << 30


def setenv(monkeypatch, *envs):
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


def registered_kinds(w):
    k = np.zeros(w.n_actors, np.uint8)
    for first, count, kind, _ in w.ranges:
        k[first:first + count] = kind
    return k


def config(w, bucket_actors=0, **cfg):
    return EngineConfig(**dict(w.gpu_kwargs(), bucket_actors=bucket_actors or w.bucket_actors, **cfg))


def counts(st):
    return st if isinstance(st, dict) else dataclasses.asdict(st) if dataclasses.is_dataclass(st) else dict(st)


class NeutralEngine(GpuEngine):
    """A GpuEngine that makes one neutral host call before every run after the first: register_range(0, 0, NONE),
    set_mailbox(0, 0, 0) and set_mailbox of actors to the class they are bound to, in turn."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.runs, self.neutral_calls, self.kinds_after = 0, [], []
        self._bound = None

    def set_mailbox(self, first, count, cls):
        self._bound = (first, count, cls)  # (a later binding overrides an earlier one: the last one holds as it stands)
        super().set_mailbox(first, count, cls)

    def neutral_call(self):
        k = len(self.neutral_calls) % 3
        if k == 0:
            GpuEngine.register_range(self, 0, 0, Kind.NONE)
        elif k == 1:
            GpuEngine.set_mailbox(self, 0, 0, 0)
        else:  # (no binding so far: every actor has class 0)
            GpuEngine.set_mailbox(self, *(self._bound or (0, self.cfg.n_actors, 0)))
        self.neutral_calls.append(k)

    def run(self, max_supersteps=QUIET, stats=True):
        if self.runs:
            self.neutral_call()
        self.runs += 1
        st = super().run(max_supersteps, stats)
        if self.cfg.n_ranks == 1:
            self.kinds_after.append(self.read_kinds())
        return st


# ================================================================== 1. neutral calls: the plain engine
BUDGETS = (2, 3, 1, QUIET)
PLAIN = {  # name -> (workload, bucket_actors): more than 8 buckets, so 3-bit digits take two passes
    "compiled20k": (lambda: wl.compiled(20_000, seed=5, throughput=2, capacity=4, builtin=True), 0),
    "compiled1200": (lambda: wl.compiled(1200, seed=5, throughput=2, capacity=4, builtin=True), 32),
    "mixed3000": (lambda: wl.mixed(3000, seed=7, throughput=2, capacity=5), 0),
}


@functools.lru_cache(maxsize=None)
def plain_reference(case):
    """the plain script on the oracle, once: (workload, bucket_actors, per leg (stats, words, alive, kinds))"""
    from oracle import BspOracle
    make, ba = PLAIN[case]
    w = make()
    ref = BspOracle(**w.engine_kwargs())
    w.apply_to(ref)
    legs = []
    for b in BUDGETS:
        so = ref.run(b)
        legs.append((so,) + ref.read_state() + (ref.read_kinds(),))
    ref.close()
    return w, ba, tuple(legs)


@pytest.mark.parametrize("pipe", list(PIPELINES))
@pytest.mark.parametrize("case", list(PLAIN))
def test_neutral_calls_plain(built, monkeypatch, case, pipe):
    w, ba, legs = plain_reference(case)
    reg = registered_kinds(w)
    so0, _, alive0, kinds0 = legs[0]
    assert so0["in_flight"] > 0, "no mail in flight at the first boundary"
    if w.behaviors is not None:  # the switch pair becomes
        assert (kinds0 != reg).any(), "no actor's kind differs from the registered one at the first boundary"
    else:                        # built-in kinds only: STOP_AFTER actors have stopped
        assert (alive0 != (reg != Kind.NONE)).any(), "no actor has stopped at the first boundary"
    assert legs[-1][0]["in_flight"] == 0
    setenv(monkeypatch, PIPELINES[pipe])
    eng = NeutralEngine(config(w, ba))
    try:
        w.apply_to(eng)
        for i, (b, (so, words, alive, kinds)) in enumerate(zip(BUDGETS, legs)):
            sg = eng.run(b)
            assert_same(sg, so, eng.read_state(), (words, alive), f"{case} {pipe} leg {i}")
            diff = np.nonzero(eng.kinds_after[-1] != kinds)[0]
            assert diff.size == 0, (f"{case} {pipe} leg {i}: {diff.size} kinds differ, first at {diff[:5]}: engine "
                                    f"{eng.kinds_after[-1][diff[:5]]} oracle {kinds[diff[:5]]} registered {reg[diff[:5]]}")
        assert eng.neutral_calls == [0, 1, 2]
    finally:
        eng.close()


# ================================================================== 1. neutral calls: the feature engines
def become_then_restart(mod, built, pipeline, launch, n):
    """supervision: test_shapes' become and restart fall into one drain window, so no kind differs at a boundary;
    here the become stands over a boundary (actors 7 and 40), then a failure restarts actor 7 to the kind it was
    registered with while actor 40 keeps the other behaviour -- the module's own workload, driver and comparisons"""
    sc = mod.sc
    E2 = 1

    def script(t):
        sc.tells(t, (7, sc.MIX_BECOME, 0), (40, sc.MIX_BECOME, 0), (9, sc.MIX_PASS, 40), (n - 2, sc.MIX_PASS, 5))
        yield t.run(1)
        sc.tells(t, (7, sc.MIX_INC, 1), (7, sc.MIX_THROW, E2), (40, sc.MIX_INC, 2))
        yield t.run(2)
        sc.tells(t, *[(a, sc.MIX_INC, 3) for a in (7, 40)], *[(a, sc.MIX_ECHO, 0) for a in (7, 40)])
        yield t.run()
    st, snap = mod.both(sc.mix_workload(n, 3), script)
    assert snap["info"]["restarts"] == 1 and snap["alive"][7] == 1 and snap["alive"][40] == 1


# feature -> (test module, test function, its arguments after `built`; "PIPE" stands for the pipeline's name): per
# feature the shortest existing script of several runs that changes kinds or per-actor device storage
FEATURES = {
    "children": ("test_gpu_children", "test_shapes", ("PIPE", "replays", 1, 128, (0, 4), 64, 4)),
    "watch": ("test_gpu_watch", "test_shapes", ("PIPE", "replays", 96)),
    "supervision": ("test_gpu_supervision", become_then_restart, ("PIPE", "replays", 96)),
    "backoff": ("test_gpu_backoff", "test_shapes", ("PIPE", "replays", 96)),
    "stash": ("test_gpu_stash", "test_population_parity", ("PIPE", 1, 1, 32)),
    "timers": ("test_gpu_timers", "test_periods", ("PIPE", (3, 16, 21), "replays", "MONKEYPATCH")),
    "receive_timeout": ("test_gpu_receive_timeout", "test_stop_turns_it_off_and_become_keeps_it", ("PIPE",)),
    "sharding": ("test_gpu_sharding", "test_random_script", ("PIPE", 1)),
    "ask": ("test_gpu_ask", "test_budgeted_runs_and_the_pump", ("PIPE",)),
    "receptionist": ("test_gpu_receptionist",
                     "test_run_ends_on_a_tick_with_changes_and_register_services_between_runs", ("PIPE", "replays")),
    "topics": ("test_gpu_topics", "test_budgets", ("PIPE", "replays")),
    "listings": ("test_gpu_listings", "test_budgets", ("PIPE", "replays")),
    "router_logics": ("test_gpu_router_logics", "test_register_services_between_runs", ("PIPE", "replays")),
}
KINDS_CHANGE = ("children", "supervision", "stash", "receive_timeout", "sharding")  # (Create, become, unstash_all, start)


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the feature modules' fixtures)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


class ModelLog:
    """what a feature's model showed after each of its runs: mail in flight, delivered, kinds"""

    def __init__(self, model):
        self.model, self.in_flight, self.delivered, self.kinds = model, [], [], []
        self.kinds0 = np.asarray(model.kind).astype(np.uint8).copy()
        run = model.run

        def logged(*a, **k):
            st = run(*a, **k)
            c = counts(st)
            self.in_flight.append(c["in_flight"])
            self.delivered.append(c["delivered"])
            self.kinds.append(np.asarray(model.kind).astype(np.uint8).copy())
            return st
        model.run = logged


@pytest.mark.parametrize("feature", list(FEATURES))
def test_neutral_calls_feature(built, monkeypatch, pipeline, feature):
    """the feature's own test -- its script, its model, its comparisons -- on an engine that makes a neutral call
    before every run after the first; on top, the kinds after every run against the model's"""
    import importlib
    mod_name, fn_name, args = FEATURES[feature]
    mod = importlib.import_module(f"tests.{mod_name}")
    engines, logs = [], []

    class Engine(NeutralEngine):
        def __init__(self, cfg):
            super().__init__(cfg)
            engines.append(self)

    model_for = mod.model_for

    def logged_model_for(*a, **k):
        m = model_for(*a, **k)
        logs.append(ModelLog(m))
        return m
    monkeypatch.setattr(mod, "GpuEngine", Engine)
    monkeypatch.setattr(mod, "model_for", logged_model_for)
    args = [pipeline if a == "PIPE" else monkeypatch if a == "MONKEYPATCH" else a for a in args]
    if callable(fn_name):
        fn_name(mod, True, *args)
    else:
        getattr(mod, fn_name)(True, *args)
    assert logs and len(engines) >= len(logs)  # (an engine without a model of its own comes first: test_budgets)
    busy = changed = False
    for eng, log in zip(engines[-len(logs):], logs):
        assert eng.runs == len(log.kinds) >= 2 and len(eng.neutral_calls) == eng.runs - 1
        for i, (g, m) in enumerate(zip(eng.kinds_after, log.kinds)):
            assert np.array_equal(g, m), (feature, i, np.nonzero(g != m)[0][:8])
        # a boundary with mail in flight, or after which the model still delivers (timers, held mail, pending asks)
        busy |= any(log.in_flight[i] > 0 or log.delivered[i + 1] > log.delivered[i] for i in range(eng.runs - 1))
        changed |= any((k != log.kinds0).any() for k in log.kinds[:-1])
    assert busy, f"{feature}: no boundary with work pending in the model"
    assert changed or feature not in KINDS_CHANGE, f"{feature}: no kind differs from the registered one at a boundary"


# ================================================================== 2. real registrations between runs
def widen(w, n_words=3):
    """the workload with `n_words` state words: every registered actor's extra words carry a value of its own"""
    ranges = []
    for first, count, kind, init in w.ranges:
        if kind != Kind.NONE:
            rows = np.zeros((count, n_words), np.uint64)
            if init is not None:
                rows[:, :init.shape[1]] = init
            for x in range(w.n_words, n_words):
                rows[:, x] = (np.uint64(0xA5 + x) << np.uint64(56)) | np.arange(first, first + count, dtype=np.uint64)
            init = rows
        ranges.append((first, count, kind, init))
    return dataclasses.replace(w, n_words=n_words, ranges=ranges)


def init_rows(first, count, n_words, salt):
    """non-zero rows, every word different"""
    rows = np.zeros((count, n_words), np.uint64)
    for x in range(n_words):
        rows[:, x] = np.uint64(salt + 3 * x + 1) + np.arange(first, first + count, dtype=np.uint64) % np.uint64(5)
    return rows


def plain_calls(w):
    """the registration calls of the legs 2 and 3 for compiled / mixed / token_ring: half of the switch (or RING)
    range unregistered; then a quarter of it registered again with a non-zero state, and ids of mixed's NONE range"""
    if w.name == "compiled":
        first, count, kind, _ = w.ranges[4]
    elif w.name == "mixed":
        first, count, kind, _ = w.ranges[1]
    else:
        first, count, kind, _ = w.ranges[0]
    again = [(first, count // 4, kind, init_rows(first, count // 4, w.n_words, 4))]
    for f, c, k, _ in w.ranges:
        if k == Kind.NONE:  # (was NONE from the start)
            again.append((f + 3, 5, Kind.COUNTER, init_rows(f + 3, 5, w.n_words, 40)))
    return [(first, count // 2, Kind.NONE, None)], again


def crdt_calls(kind, delta=False):
    def calls(w):
        n, W = w.n_actors, w.n_words
        rows = np.zeros((16, W), np.uint64)
        if delta:  # (the replicas go on writing: small values, a valid ORSet; envelope and log start empty)
            if kind == Kind.ORSET:
                from oracle.oracle import orset
                rows[:, :CRDT_WORDS[kind]] = orset.add(orset.add(orset.add(orset.empty(), 1, 5), 2, 9), 1, 40)
            else:
                rows[:, :CRDT_WORDS[kind]] = init_rows(0, 16, CRDT_WORDS[kind], 7)
        elif kind == Kind.ORSET:  # crafted states: versions up to 2^32 - 1 (these replicas only merge)
            rows[:] = C.orset_words(C.population(16))
        else:
            rows[:] = C.counter_population(kind, 16)
        first = n // 8 + 4  # (not the writers 0..7; a range that straddles nothing special but no bucket start either)
        return [(0, n // 2, Kind.NONE, None)], [(first, 16, kind, rows)]
    return calls


REG = {  # name -> (workload, bucket_actors, env, calls)
    "compiled20k": (PLAIN["compiled20k"][0], 0, {}, plain_calls),
    "compiled1200": (PLAIN["compiled1200"][0], 32, {}, plain_calls),
    "mixed3000": (PLAIN["mixed3000"][0], 0, {}, plain_calls),
    "ring1200_w1": (lambda: wl.token_ring(1200, 9, throughput=2, tokens_per_actor=2), 32, {}, plain_calls),
    "compiled1200_soa": (PLAIN["compiled1200"][0], 32, {"AGX_STATE_SOA": "1"}, plain_calls),
    "mixed3000_soa": (PLAIN["mixed3000"][0], 256, {"AGX_STATE_SOA": "1"}, plain_calls),
    "compiled1200_w3": (lambda: widen(PLAIN["compiled1200"][0]()), 32, {}, plain_calls),
    "mixed3000_w3": (lambda: widen(PLAIN["mixed3000"][0]()), 256, {}, plain_calls),
}
CRDT_NAMES = {Kind.GCOUNTER: "gcounter", Kind.PNCOUNTER: "pncounter", Kind.ORSET: "orset"}
for _kind, _name in CRDT_NAMES.items():
    for _lay in ("unset", "actor", "word"):
        REG[f"{_name}_{_lay}"] = (functools.partial(wl.crdt_gossip, 3000, _kind, rounds=8, throughput=2), 0,
                                  {} if _lay == "unset" else {"AGX_CRDT_LAYOUT": _lay}, crdt_calls(_kind))
    for _lay in ("unset", "actor"):  # the delta engines at their tests' smallest size
        REG[f"delta_{_name}_{_lay}"] = (functools.partial(wl.crdt_delta, 8 * 100 + 3, _kind, rounds=6, write=True,
                                                          ops_per_replica=3, gossip_rounds=2, throughput=2), 0,
                                        {} if _lay == "unset" else {"AGX_CRDT_LAYOUT": _lay}, crdt_calls(_kind, delta=True))


def distinct_gcounters():
    """crdt_gossip's GCounter replicas from states that tell the replicas apart, both u32 halves in use (the max of
    any slot stays far from 2^64: the writers go on incrementing)"""
    w = wl.crdt_gossip(3000, Kind.GCOUNTER, rounds=8, throughput=2)
    ids = np.arange(w.n_actors, dtype=np.uint64)
    rows = np.stack([((ids * np.uint64(2654435761) % np.uint64(1 << 20)) << np.uint64(20 + x)) | (ids + np.uint64(x))
                     for x in range(w.n_words)], axis=1)
    return dataclasses.replace(w, ranges=[(0, w.n_actors, Kind.GCOUNTER, rows)])


REG["gcounter_rows"] = (distinct_gcounters, 0, {}, crdt_calls(Kind.GCOUNTER))
REG_LEGS = (2, 1, QUIET)


def run_legs(target, w, calls, run=None, kinds=True):
    """the three legs on one target: per leg (stats, words, alive, kinds or None)"""
    run = run or (lambda b: target.run(b))
    out = []
    for b, regs in zip(REG_LEGS, ((),) + tuple(calls)):
        for first, count, kind, init in regs:
            target.register_range(first, count, kind, init)
        st = run(b)
        out.append((counts(st),) + tuple(target.read_state()) + (target.read_kinds() if kinds else None,))
    return out


def assert_preconditions(legs, plain, name):
    """on the reference: mail in flight at the first boundary, dead letters made by the unregistering leg, and a run
    that ends elsewhere than the uninterrupted one"""
    assert legs[0][0]["in_flight"] > 0, f"{name}: no mail in flight at the first boundary"
    assert legs[1][0]["dead_letters"] > plain[1]["dead_letters"], f"{name}: the unregistering leg made no dead letters"
    assert legs[2][0]["in_flight"] == 0
    assert any(legs[2][0][k] != plain[2][k] for k in COUNT_KEYS), f"{name}: the registrations changed no counter"


@functools.lru_cache(maxsize=None)
def reg_reference(case):
    """the three legs on the oracle, once: (workload, per leg (stats, words, alive, kinds))"""
    from oracle import BspOracle
    make, ba, env, calls = REG[case]
    w = make()
    ref = BspOracle(**w.engine_kwargs())
    w.apply_to(ref)
    legs = run_legs(ref, w, calls(w))
    ref.close()
    ref = BspOracle(**w.engine_kwargs())  # the uninterrupted run, same budgets
    w.apply_to(ref)
    plain = [ref.run(b) for b in REG_LEGS]
    ref.close()
    assert_preconditions(legs, plain, case)
    return w, legs


def check_registrations(case, name):
    make, ba, env, calls = REG[case]
    w, legs = reg_reference(case)
    eng = GpuEngine(config(w, ba))
    try:
        w.apply_to(eng)
        got = run_legs(eng, w, calls(w))
    finally:
        eng.close()
    for i, (g, r) in enumerate(zip(got, legs)):
        for k in COUNT_KEYS:
            assert g[0][k] == r[0][k], f"{name} leg {i}: {k} gpu={g[0][k]} oracle={r[0][k]}"
        assert np.array_equal(g[2], r[2]), f"{name} leg {i}: alive differs at {np.nonzero(g[2] != r[2])[0][:8]}"
        diff = np.nonzero((g[1] != r[1]).any(axis=1))[0]
        assert diff.size == 0, f"{name} leg {i}: state differs at {diff[:10]} gpu={g[1][diff[:2]]} oracle={r[1][diff[:2]]}"
        diff = np.nonzero(g[3] != r[3])[0]
        assert diff.size == 0, f"{name} leg {i}: kinds differ at {diff[:10]} gpu={g[3][diff[:5]]} oracle={r[3][diff[:5]]}"


@pytest.mark.parametrize("pipe", list(PIPELINES))
@pytest.mark.parametrize("case", ["compiled20k", "compiled1200", "mixed3000"])
def test_registrations_pipelines(built, monkeypatch, case, pipe):
    setenv(monkeypatch, PIPELINES[pipe], REG[case][2])
    check_registrations(case, f"{case} {pipe}")


@pytest.mark.parametrize("pipe", list(PIPELINES))
@pytest.mark.parametrize("case", [c for c in REG if c not in ("compiled20k", "compiled1200", "mixed3000")])
def test_registrations_layouts(built, monkeypatch, case, pipe):
    """n_words 1, 2 as pairs (above) and word-major (AGX_STATE_SOA), 3; CRDT rows actor-major with a padded pitch
    and word-major, full-state and delta"""
    setenv(monkeypatch, PIPELINES[pipe], REG[case][2])
    check_registrations(case, f"{case} {pipe}")


def test_registrations_lwwmap(built, pipeline):
    """LWWMap replicas against LwwModel: the re-registered replicas start from crafted maps of two puts"""
    from tests import lwwmap_model as L
    w = wl.crdt_lwwmap(96, rounds=8, throughput=2, bucket_actors=32)

    # two puts each, keys the writers use too, timestamps around and above the run's logical time
    rows = np.stack([L.to_words(L.LWWMap().put(i % 8, i % 12, 1000 + i, L.default_clock, 3 + 4 * i)
                                .put((i + 3) % 8, (i + 5) % 12, 7 + i, L.default_clock, 60)) for i in range(16)])

    def legs_of(target):
        out = []
        w.apply_to(target)
        for leg, b in enumerate(REG_LEGS):
            if leg == 1:
                target.register_range(0, 48, Kind.NONE)
            if leg == 2:
                target.register_range(12, 16, Kind.LWWMAP, rows)
            st = counts(target.run(b))
            out.append((st,) + tuple(target.read_state()))
        return out
    want = legs_of(L.LwwModel(**w.engine_kwargs()))
    plain = L.LwwModel(**w.engine_kwargs())
    w.apply_to(plain)
    assert_preconditions(want, [counts(plain.run(b)) for b in REG_LEGS], "lwwmap")
    eng = GpuEngine(config(w))
    try:
        got = legs_of(eng)
    finally:
        eng.close()
    for i, (g, m) in enumerate(zip(got, want)):
        for k in COUNT_KEYS:
            assert g[0][k] == m[0][k], (i, k, g[0][k], m[0][k])
        assert np.array_equal(g[2] & 1, m[2] & 1), i
        diff = np.nonzero((g[1][:, :L.LWWMAP_WORDS] != m[1][:, :L.LWWMAP_WORDS]).any(axis=1))[0]
        assert diff.size == 0, (i, diff[:10])


RANKS = 3


def owned_merge(engs, n, read):
    """each rank's rows of the ids it owns, merged (as test_loopback_sharded)"""
    own_of = np.array([owner(i, 1000, len(engs)) for i in range(n)])
    words = alive = None
    for e in engs:
        a, b = read(e)
        if words is None:
            words, alive = np.zeros_like(a), np.zeros_like(b)
        own = own_of == e.cfg.rank
        words[own], alive[own] = a[own], b[own]
    return words, alive


def test_registrations_loopback_ranks(built):
    """R = 3 loopback ranks: the same registration calls on every rank's engine"""
    from oracle import BspOracle
    make, ba, env, calls = REG["mixed3000"]
    w = make()

    class Group:  # (the oracle's interface over the ranks' engines)
        def __init__(self, engs):
            self.engs = engs

        def register_range(self, *a):
            for e in self.engs:
                e.register_range(*a)

        def read_state(self):
            return owned_merge(self.engs, w.n_actors, lambda e: e.read_state())

    ref = BspOracle(n_ranks=RANKS, **w.engine_kwargs())
    w.apply_to(ref)
    legs = run_legs(ref, w, calls(w), kinds=False)
    ref.close()
    ref = BspOracle(n_ranks=RANKS, **w.engine_kwargs())
    w.apply_to(ref)
    assert_preconditions(legs, [ref.run(b) for b in REG_LEGS], "mixed3000 R=3")
    ref.close()
    engs = [GpuEngine(config(w, n_ranks=RANKS, rank=r)) for r in range(RANKS)]
    try:
        for e in engs:
            w.apply_to(e)
        got = run_legs(Group(engs), w, calls(w), run=lambda b: GpuEngine.group_run(engs, b), kinds=False)
    finally:
        for e in engs:
            e.close()
    for i, (g, r) in enumerate(zip(got, legs)):
        for k in SHARDED_KEYS:
            assert g[0][k] == r[0][k], (i, k, g[0][k], r[0][k])
        assert np.array_equal(g[2], r[2]), (i, np.nonzero(g[2] != r[2])[0][:8])
        diff = np.nonzero((g[1] != r[1]).any(axis=1))[0]
        assert diff.size == 0, (i, diff[:10])


# ================================================================== 3. reads
@pytest.mark.parametrize("case", ["compiled1200", "compiled1200_w3", "gcounter_rows"])
def test_reads_while_the_mirror_is_newer(built, case):
    """read_kinds / read_state after a register_range and before the next run: untouched actors show what the device
    left (becomes, stops), registered ones the new kind and state"""
    from oracle import BspOracle
    make, ba, env, calls = REG[case]
    w = make()
    reg = registered_kinds(w)
    (first, count, kind, rows), = calls(w)[1][:1]
    ref = BspOracle(**w.engine_kwargs())
    eng = GpuEngine(config(w, ba))
    try:
        for t in (ref, eng):
            w.apply_to(t)
            t.run(2)
            t.register_range(first, count, kind, rows)
        kinds, (words, alive) = ref.read_kinds(), ref.read_state()
        untouched = np.ones(w.n_actors, bool)
        untouched[first:first + count] = False
        if w.behaviors is not None:
            assert (kinds[untouched] != reg[untouched]).any(), "no untouched actor has become another behaviour"
            assert (alive[untouched] != (reg[untouched] != 0)).any(), "no untouched actor has stopped"
        assert (words[untouched] != 0).any() and np.array_equal(words[first:first + count], rows)
        assert (kinds[first:first + count] == kind).all() and alive[first:first + count].all()
        for _ in range(2):  # (a read changes nothing: the second one sees the same)
            assert np.array_equal(eng.read_kinds(), kinds)
            gw, ga = eng.read_state()
            assert np.array_equal(ga, alive) and np.array_equal(gw, words)
        so, sg = ref.run(), eng.run()
        assert_same(sg, so, eng.read_state(), ref.read_state(), f"{case} after the reads")
        assert np.array_equal(eng.read_kinds(), ref.read_kinds())
    finally:
        eng.close()
        ref.close()


SENTINEL_WORD, SENTINEL_FLAG = 0xDEADBEEFCAFEF00D, 0xEE


def read_into(eng, first, count):
    """agx_read_state into buffers filled with a sentinel: rows the call does not write stay as they were passed"""
    words = np.full((count, eng.cfg.n_words), SENTINEL_WORD, np.uint64)
    alive = np.full(count, SENTINEL_FLAG, np.uint8)
    from akka_amd._lib import check
    check(eng.lib.agx_read_state(eng.handle, first, count, words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                 alive.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
    return words, alive


def sub_ranges(n, ba):
    return [(0, 1), (ba - 1, 2), (ba, ba), (n - 3, 3), (n, 0)]


def check_sub_ranges(eng, n, ba, full):
    for first, count in sub_ranges(n, ba):
        assert first + count <= n
        words, alive = read_into(eng, first, count)
        assert np.array_equal(words, full[0][first:first + count]), (first, count)
        assert np.array_equal(alive, full[1][first:first + count]), (first, count)
    for first, count in ((n - 1, 2), (n + 1, 0), (0, n + 1)):
        with pytest.raises(AgxError):
            eng.read_state(first, count)


@pytest.mark.parametrize("case,ba,steps", [("compiled1200", 32, 2), ("compiled1200_w3", 32, 2), ("gcounter_rows", 512, 3)])
def test_read_state_sub_ranges(built, case, ba, steps):
    """agx_read_state(first, count) is the slice of the full read: with mail in flight after a run (the device is
    the newer side) and after a registration (the mirror is)"""
    from oracle import BspOracle
    make, _, env, calls = REG[case]
    w = make()
    ref = BspOracle(**w.engine_kwargs())
    eng = GpuEngine(config(w, ba))
    try:
        for t in (ref, eng):
            w.apply_to(t)
        so, sg = ref.run(steps), eng.run(steps)
        assert so["in_flight"] > 0 and sg.in_flight == so["in_flight"]
        for leg in range(2):
            want = ref.read_state()
            full = read_into(eng, 0, w.n_actors)
            assert np.array_equal(full[0], want[0]) and np.array_equal(full[1], want[1]), leg
            assert len(np.unique(want[0], axis=0)) > 8, "the rows do not tell the actors apart"
            check_sub_ranges(eng, w.n_actors, ba, full)
            for t in (ref, eng):
                t.register_range(*calls(w)[1][0])
    finally:
        eng.close()
        ref.close()


def test_read_state_sub_ranges_ranks(built):
    """R = 3: a rank writes the rows of the ids it owns, the others stay as the caller passed them"""
    from oracle import BspOracle
    ba = 256
    w = PLAIN["mixed3000"][0]()
    n = w.n_actors
    ref = BspOracle(n_ranks=RANKS, **w.engine_kwargs())
    w.apply_to(ref)
    assert ref.run(2)["in_flight"] > 0
    want = ref.read_state()
    ref.close()
    own_of = np.array([owner(i, 1000, RANKS) for i in range(n)])
    engs = [GpuEngine(config(w, ba, n_ranks=RANKS, rank=r)) for r in range(RANKS)]
    try:
        for e in engs:
            w.apply_to(e)
        GpuEngine.group_run(engs, 2)
        for e in engs:
            own = own_of == e.cfg.rank
            assert 0 < own.sum() < n
            full = read_into(e, 0, n)
            assert np.array_equal(full[0][own], want[0][own]) and np.array_equal(full[1][own], want[1][own])
            assert (full[0][~own] == SENTINEL_WORD).all() and (full[1][~own] == SENTINEL_FLAG).all()
            check_sub_ranges(e, n, ba, full)
    finally:
        for e in engs:
            e.close()
