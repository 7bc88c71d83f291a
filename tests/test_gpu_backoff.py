"""restartWithBackoff on the GPU (agx_set_backoff; TY/internal/Supervision.scala:163-406): the HIP engine through the
C ABI against the known answers worked out from the reference's SupervisionSpec (tests/golden/backoff_kats.json) and
against the model of DESIGN.md §2.14 (tests/backoff_model.py, itself pinned to the known answers by
tests/test_backoff_model.py), on the fused and the multi-pass pipelines, with graph replays and eager launches.
Everything is compared bit for bit after every run: states, alive flags, kinds, every counter, the outbox order,
supervision_info, backoff_info, read_supervision and read_backoff of every actor, and conservation.  Every test
calls agx_set_backoff."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import EngineConfig, GpuEngine
from tests import backoff_cases as bc
from tests import supervision_cases as sc
from tests.backoff_model import BackoffModel
from tests.supervision_model import SupervisionModel

pytestmark = pytest.mark.gpu

E1, E2, E3 = bc.E1, bc.E2, bc.E3
THROW, STOP, INC, ECHO, TO = bc.MIX_THROW, bc.MIX_STOP, bc.MIX_INC, bc.MIX_ECHO, bc.MIX_TO
PAIR = (16, 17)   # the ticker pair of the mix population


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the supervision tests' fixture; NO_FUSED: populations of one digit)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


@pytest.fixture(params=["replays", "eager"])
def launch(request, monkeypatch):
    if request.param == "eager":
        monkeypatch.setenv("AGX_NO_GRAPH", "1")
    return request.param


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def model_for(w, cls=BackoffModel):
    m = cls(**w.engine_kwargs())
    w.apply_to(m)
    return m


def conserved(st):
    return st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def both(w, script, actors=None):
    """run `script(target)` -- a generator that yields after every run's stats -- on the engine and the model and
    compare everything after every run; returns the last stats and snapshot, the outbox that of all runs"""
    eng, mod = engine_for(w), model_for(w)
    actors = range(w.n_actors) if actors is None else actors
    n = 0
    sent = []
    for sg, sm in zip(script(eng), script(mod)):
        sg, sm = bc.counts(sg), bc.counts(sm)
        assert sg == sm, (n, sg, sm)
        g, m = bc.snapshot(eng, actors), bc.snapshot(mod, actors)
        for k in g:
            assert g[k] == m[k], (n, k, g[k], m[k])
        assert np.array_equal(eng.read_kinds(), mod.kind.astype(np.uint8))
        assert conserved(sg) and g["info"]["ticks"] == sg["supersteps"]
        assert g["backoff"]["resumed"] + g["backoff"]["suspended"] == g["backoff"]["backoffs"]
        sent += list(zip(*m["outbox"]))
        n += 1
    eng.close()
    m["outbox"] = sorted(sent, key=lambda x: x[0])   # (stable: every sender's envelopes in emission order)
    return sm, m


# ------------------------------------------------------------------ 1. the known answers
@pytest.mark.parametrize("T", bc.KAT_T)
@pytest.mark.parametrize("name", bc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(bc.kat_workload(name, T))
    got = bc.run_kat(name, T, eng)
    eng.close()
    print(got)
    bc.check_kat(name, T, got)
    assert got == bc.run_kat(name, T, model_for(bc.kat_workload(name, T)))


# ------------------------------------------------------------------ 2. shapes: buckets, windows, backlogs
def shapes_script(n):
    """three buckets of 32 (the last one partial at 70), throughput 3: a failure in the first and the last actor of
    every bucket; as the first, a middle and the last message of a window; with a backlog already queued; in two
    actors of one thread's four in the same tick; while the held mail is drained (a second failure, the doubled
    delay); an uncaught class and a `stopped` behind held mail"""
    edge = sorted({0, 31, 32, 63, 64, n - 1})

    def script(t):
        bc.tells(t, *[(a, INC, 7) for a in edge], *[(a, THROW, E1) for a in edge], *[(a, INC, 8) for a in edge],
                 (5, THROW, E1), (5, INC, 1), (5, INC, 2), (5, ECHO, 0),                   # the first of a window
                 (6, INC, 1), (6, THROW, E2), (6, INC, 2), (6, ECHO, 0),                   # a middle one
                 (7, INC, 1), (7, INC, 2), (7, THROW, E1), (7, INC, 3), (7, ECHO, 0),      # the last one
                 *[(8, INC, i) for i in range(4)], (8, THROW, E1), *[(8, INC, i) for i in range(3)], (8, ECHO, 0),  # a backlog
                 # two of the four actors one thread classifies and requeues (blocked: 12..15); the drain takes actors
                 # striped, one per thread in a bucket of 32: test_two_actors_of_one_drain_thread has that side
                 (12, THROW, E1), (12, INC, 1), (13, INC, 1), (13, THROW, E1), (13, ECHO, 0),
                 (9, THROW, E1), (9, THROW, E2), (9, INC, 1), (9, ECHO, 0),                # a failure in the held mail
                 (10, THROW, E1), (10, THROW, E3), (10, INC, 1),                           # ... an uncaught one: stops
                 (11, THROW, E1), (11, STOP, 0), (11, INC, 1))                             # ... a stop
        bc.mix_tick(t, 12, PAIR)
        yield t.run(1)
        yield t.run(2)
        bc.tells(t, (5, INC, 9), (8, INC, 9), (n - 1, ECHO, 0))     # arrivals behind held mail
        yield t.run(3)
        yield t.run()
    return script


@pytest.mark.parametrize("n", [96, 70])
def test_shapes(built, pipeline, launch, n):
    sup = (("E1", bc.backoff(2, 8, reset_after=50)),)
    st, snap = both(bc.mix_workload(n, 3, sup), shapes_script(n))
    assert snap["backoff"]["backoffs"] >= 13 and snap["backoff"]["suspended"] == 0 and st["in_flight"] == 0
    assert snap["sup"][9][1][0] == 2 and [snap["alive"][a] for a in (9, 10, 11)] == [1, 0, 0]
    assert snap["words"][8][0] == 4    # the three Incs behind the failure and the later arrival, in the restarted state


def test_two_actors_of_one_drain_thread(built, pipeline, launch):
    """one bucket of 2048 (partial: 1100 actors): the drain takes actors striped over 512 threads, so actors 5, 517 and
    1029 are one thread's; all three fail in the same tick, at different places of their windows, beside a fourth
    that does not"""
    n, mine = 1100, (5, 517, 1029)
    sup = (("E1", bc.backoff(2, 8, stash=2)),)

    def script(t):
        bc.tells(t, (5, THROW, E1), (5, INC, 1), (5, INC, 2), (5, INC, 3), (5, ECHO, 0),
                 (517, INC, 1), (517, THROW, E1), (517, INC, 2), (517, ECHO, 0),
                 (1029, INC, 1), (1029, INC, 2), (1029, THROW, E2), (1029, ECHO, 0), (1029, INC, 3), (1029, INC, 4),
                 (6, INC, 1), (518, INC, 1), (1099, THROW, E1), (1099, ECHO, 0))
        yield t.run(1)
        bc.tells(t, (5, ECHO, 0), (517, INC, 5), (1029, ECHO, 0))
        yield t.run()
    st, snap = both(bc.mix_workload(n, 3, sup, bucket_actors=2048), script, actors=mine + (6, 518, 1099))
    # stash 2: actor 5 holds two of the four behind its failure and loses its Echo of tick 2, 517 holds both and loses
    # the Inc of tick 2, 1029 holds two of three and loses its Echo; 1099 holds its one
    assert snap["backoff"]["backoffs"] == 4 and snap["backoff"]["dropped"] == 3 + 1 + 2 and st["in_flight"] == 0
    assert [snap["words"][a][0] for a in mine] == [2, 1, 1]


# ------------------------------------------------------------------ 3. the stash bound
@pytest.mark.parametrize("stash", [0, 1, 2, 5, -1])
def test_stash_capacities(built, pipeline, launch, stash):
    """mailbox capacity 4, stash capacities 0, 1, 2, one above the mailbox capacity and the mailbox capacity itself:
    the cut at the failure, then arrivals from three senders in one tick racing the bound, twice"""
    n = 96
    init = np.zeros((n, 2), np.uint64)
    init[20:23, 1] = 40
    init[52:55, 1] = 63
    sup = (("E1", bc.backoff(6, 6, stash=stash)),)

    def script(t):
        bc.tells(t, (40, THROW, E1), (40, INC, 1), (40, INC, 2), (40, INC, 3),
                 (63, INC, 1), (63, THROW, E1), (63, INC, 2))
        bc.mix_tick(t, 10, PAIR)
        yield t.run(1)
        for k in range(2):
            bc.tells(t, *[(a, TO, 10 * k + a) for a in (20, 21, 22, 52, 53, 54)])
            yield t.run(2)   # the senders' tick, then the arrivals'
        bc.tells(t, (40, ECHO, 0), (63, ECHO, 0))
        yield t.run()
    st, snap = both(bc.mix_workload(n, 3, sup, capacity=4, init=init), script)
    bound = 4 if stash in (5, -1) else stash     # (what either actor holds at most)
    held = min(3, bound) + min(1, bound)          # ... after the cut at the failure
    # behind the failures 3 + 1 messages, then 2 * 3 arrivals and the Echo each, all before `until` = 7
    assert snap["backoff"]["dropped"] == 4 + 12 + 2 - 2 * bound and st["dead_letters"] == snap["backoff"]["dropped"]
    assert snap["backoff"]["backoffs"] == 2 and st["in_flight"] == 0 and held <= 2 * bound


# ------------------------------------------------------------------ 4. time: held mail carries it, an empty queue does not
def test_held_mail_lets_the_delay_pass(built, pipeline, launch):
    """a suspended actor alone with held mail, run to quiescence: the held mail is in flight, so the ticks go on until
    the delay has passed, and the mail is processed in order"""
    sup = (("E1", bc.backoff(5, 5)),)

    def script(t):
        bc.tells(t, (40, INC, 1), (40, THROW, E1), (40, ECHO, 0), (40, INC, 2), (40, INC, 3), (40, ECHO, 0))
        yield t.run()
    st, snap = both(bc.mix_workload(96, 2, sup), script)
    assert st["supersteps"] == 7 and st["in_flight"] == 0       # the failure at tick 1, `until` 6, two ticks of two
    assert [p & 0xFFFFFF for s, d, p in snap["outbox"] if s == 40] == [1, 0, 2]   # PreRestart(1), Echo(0), Echo(2)


def test_time_does_not_pass_without_mail(built, pipeline, launch):
    """a suspended actor with an empty queue across two runs: no mail, no tick, it stays suspended"""
    sup = (("E1", bc.backoff(4, 4)),)
    seen = []

    def script(t):
        bc.tells(t, (40, THROW, E1))
        yield t.run()
        seen.append((t.read_backoff(40), t.backoff_info()["suspended"]))
        yield t.run()
        seen.append((t.read_backoff(40), t.backoff_info()["suspended"]))
        bc.tells(t, (40, INC, 1), (40, ECHO, 0))
        yield t.run()
    st, snap = both(bc.mix_workload(96, 3, sup), script)
    assert seen[0] == seen[1] == seen[2] == seen[3] == (dict(suspended_for=3, until=5), 1)
    assert st["supersteps"] == 5 and snap["words"][40][0] == 1 and snap["backoff"]["suspended"] == 0


# ------------------------------------------------------------------ 5. a bucket without suspended actors beside one with
def test_quiet_buckets_beside_a_suspended_one(built, pipeline, launch):
    sup = (("E1", bc.backoff(3, 12, reset_after=2)),)

    def script(t):
        for k in range(3):
            bc.tells(t, *[(a, INC, k) for a in range(0, 96, 5)], (40, THROW, E1), (40, INC, k), (50, THROW, E2))
            bc.mix_tick(t, 8, PAIR)
            yield t.run(4)
        yield t.run()
    st, snap = both(bc.mix_workload(96, 3, sup), script)
    assert snap["backoff"]["backoffs"] >= 4 and all(snap["bo"][a] == (("suspended_for", 0), ("until", 0)) for a in range(32))


# ------------------------------------------------------------------ 6. nesting, the limit
@pytest.mark.parametrize("order", ["inner_backoff", "outer_backoff"])
def test_nesting(built, pipeline, launch, order):
    """an outer restart clears the inner backoff entry's count and reset-due, and the reverse"""
    bo = bc.backoff(1, 8, reset_after=50)
    sup = (("E2", bo), ("E1", "restart")) if order == "inner_backoff" else (("E2", "restart"), ("E1", bo))

    def script(t):
        for cls in (E2, E2, E1, E2, E1, E1):
            bc.tells(t, (33, INC, 1), (33, THROW, cls), (33, ECHO, 0))
            bc.mix_tick(t, 10, PAIR)
            yield t.run()
    st, snap = both(bc.mix_workload(70, 3, sup), script)
    assert snap["info"]["restarts"] == 6 and snap["info"]["stops"] == 0
    # the last failure is the outer entry's and clears the inner count; the plain outer restart's window of one tick
    # has run out each time (count 1), the outer backoff entry's reset-due has not (count 3)
    assert snap["sup"][33][1][:2] == ([0, 1] if order == "inner_backoff" else [0, 3])
    assert snap["backoff"]["backoffs"] == 3


def test_limit_is_not_rethrown_to_an_outer_resume(built, pipeline, launch):
    """withMaxRestarts(1) reached: the actor stops, although an outer entry would resume the class"""
    sup = (("E1", bc.backoff(1, 1, max_restarts=1, reset_after=50)), ("E1", "resume"))

    def script(t):
        for _ in range(2):
            bc.tells(t, (3, INC, 1), (3, THROW, E1), (64, THROW, E1))
            yield t.run()
    st, snap = both(bc.mix_workload(96, 3, sup), script)
    assert snap["info"]["resumes"] == 0 and snap["info"]["stops"] == 2 and snap["backoff"]["limit_stops"] == 2
    assert snap["alive"][3] == 0 and snap["alive"][64] == 0


# ------------------------------------------------------------------ 7. plain rows: the supervision engine's results
@pytest.mark.parametrize("n", [96, 70])
def test_plain_rows_are_the_supervision_engine(built, pipeline, launch, n):
    """agx_set_backoff with rows that are all plain: the backoff instantiation runs and gives, bit for bit, what the
    supervision engine and the supervision model give"""
    w = sc.mix_workload(n, 3)
    plain = wl.Workload(**dict(w.__dict__, supervision=dict(w.supervision, backoff=[[typed.AgxBackoff()] for _ in w.supervision["rows"]])))
    assert not plain.behaviors.uses_backoff
    snaps = []
    for wk, cls in ((plain, BackoffModel), (w, SupervisionModel)):
        eng, mod = engine_for(wk), model_for(wk, cls)
        for sg, sm in zip(sc.shapes_script(n)(eng), sc.shapes_script(n)(mod)):
            assert sc.counts(sg) == sc.counts(sm)
            g, m = sc.snapshot(eng, range(n)), sc.snapshot(mod, range(n))
            assert g == m
            snaps.append(g)
        if wk is plain:
            assert eng.backoff_info() == dict(backoffs=0, resumed=0, dropped=0, limit_stops=0, suspended=0)
        eng.close()
    assert snaps[:len(snaps) // 2] == snaps[len(snaps) // 2:]


# ------------------------------------------------------------------ 8. the workloads
@pytest.mark.parametrize("name", ["backoff_workers", "backoff_stash_pressure"])
def test_workloads(built, pipeline, name):
    w = wl.backoff_workers(1 << 12, jobs=6, hops=4) if name == "backoff_workers" else wl.backoff_stash_pressure(1 << 12, ticks=16)

    def script(t):
        yield t.run(5)
        yield t.run()
    st, snap = both(w, script, actors=range(0, w.n_actors, 97))
    assert snap["backoff"]["backoffs"] > 100 and st["in_flight"] == 0
    if name == "backoff_workers":
        assert max(c[1][0] for c in snap["sup"]) > 3    # the counts pass 3
    else:
        assert snap["backoff"]["dropped"] > 100
