"""The model of the ask pattern (tests/ask_model.py) against the known answers restated from the
reference's ActorContextAskSpec and AskSpec (tests/golden/ask_kats.json) and one case per rule of the contract, the
bounded differences included.  No GPU: the GPU file compares the engine with this model snapshot for snapshot."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from tests import ask_cases as ac
from tests.ask_model import AskModel, ask_ref
from tests.timer_model import TimerModel

P = ac.payload


def make(w):
    m = AskModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


@pytest.mark.parametrize("T", ac.KAT_T)
@pytest.mark.parametrize("name", ac.KAT_NAMES)
def test_kat(name, T):
    got = ac.run_kat(name, T, make(ac.kat_workload(name, T)))
    ac.check_kat(name, T, got)


def test_kats_cite_the_reference():
    assert all(s["cite"].split(".scala:")[0] in ("ActorContextAskSpec", "AskSpec") for s in ac.KATS["scenarios"])
    assert len(ac.KAT_NAMES) == 7


@pytest.mark.parametrize("T", (1, 4))
def test_reply_and_timeout_due_in_one_tick(T):
    (s,) = ac.case_reply_and_timeout_in_one_tick(make, T)
    assert ac.echoes(s) == [P("Adapted:5")]  # the reply is first in the inbox of tick 3 and wins
    assert s["info"] == dict(asked=1, answered=1, timed_out=0, late=0)
    assert s["timer_info"]["fired"] == 1 and s["timer_info"]["discarded"] == 1  # the timeout that lost is a stale TimerMsg
    assert s["timer_info"]["ticks"] == (4 if T == 1 else 3)  # (throughput 1: the TimerMsg waits a tick in the backlog)


@pytest.mark.parametrize("T", (1, 4))
def test_t1_always_times_out(T):
    (s,) = ac.case_t1_against_prompt_target(make, T)
    assert ac.echoes(s) == [P("TimedOut")] and s["info"] == dict(asked=1, answered=0, timed_out=1, late=1)
    assert s["counts"]["unhandled"] == 0 and s["timer_info"]["ticks"] == 3


def test_late_reply_after_timeout():
    a, b = ac.case_late_reply_after_timeout(make, 4)
    assert ac.echoes(a) == [P("TimedOut")] and a["info"] == dict(asked=1, answered=0, timed_out=1, late=0)
    assert ac.echoes(b) == [] and b["info"]["late"] == 1 and b["counts"]["unhandled"] == 0
    assert b["words"][ac.ACTOR][0] == 1  # (the behaviour did not run on the late reply)


def test_two_replies_to_one_ask():
    _, s = ac.case_two_replies(make, 4)
    assert ac.echoes(s) == [P("Adapted:1")] and s["info"] == dict(asked=1, answered=1, timed_out=0, late=1)


def test_supersede_on_one_key():
    """bounded difference 1: at most n_keys outstanding asks, asking again on a key supersedes"""
    (s,) = ac.case_supersede(make, 1)
    assert ac.echoes(s) == [P("Adapted:2")] and s["info"] == dict(asked=2, answered=1, timed_out=0, late=1)
    assert s["timer_info"]["fired"] == 0


def test_cancel_and_cancel_all_abandon_the_ask():
    (s,) = ac.case_cancel(make, 1)
    assert ac.echoes(s) == [] and s["info"] == dict(asked=1, answered=0, timed_out=0, late=1) and s["timer_info"]["fired"] == 0
    (s,) = ac.case_cancel_all(make, 1)
    assert ac.echoes(s) == [] and s["info"] == dict(asked=2, answered=0, timed_out=0, late=2) and s["timer_info"]["fired"] == 0


def test_asker_stops_with_an_ask_outstanding():
    (s,) = ac.case_asker_stops(make, 1)
    assert s["alive"][ac.ACTOR] == 0 and s["info"] == dict(asked=1, answered=0, timed_out=0, late=0)
    assert s["counts"]["dead_letters"] == 1 and s["timer_info"]["active"] == 0 and s["timer_info"]["fired"] == 0


def test_target_keeps_the_ref_and_answers_later():
    a, b = ac.case_keeper_answers_later(make, 4)
    ref = ask_ref(0, 1, ac.ACTOR)  # key 0, the actor's first generation
    assert a["words"][ac.TARGET][1] == ref and a["slots"][ac.ACTOR][5][0] == 1 and a["slots"][ac.ACTOR][6][0] == ac.TAGS["Adapted"]
    assert a["slots"][ac.ACTOR][1][0] == 1 + 9 - 5 and a["timer_info"]["pending"] == 1  # (asked in tick 1, 5 ticks run)
    assert ac.echoes(b) == [P("Adapted:6")] and b["info"] == dict(asked=1, answered=1, timed_out=0, late=0)
    assert b["slots"][ac.ACTOR][5] == [0] * 4 and b["timer_info"]["fired"] == 0


def test_full_bounded_mailbox_kills_the_reply():
    """bounded difference 3: the reply dies at the full mailbox and the timeout follows"""
    _, s = ac.case_full_mailbox_kills_reply(make, 4)
    assert ac.echoes(s) == [P("TimedOut")] and s["info"] == dict(asked=1, answered=0, timed_out=1, late=0)
    assert s["counts"]["dead_letters"] == 1


def test_ask_and_plain_timer_on_neighbouring_keys():
    (s,) = ac.case_ask_and_plain_timer(make, 4)
    assert ac.echoes(s) == [P("Adapted:5"), P("PlainFired")] and s["info"] == dict(asked=1, answered=1, timed_out=0, late=0)
    assert s["timer_info"]["fired"] == 1 and s["timer_info"]["discarded"] == 0


def test_reply_addressed_to_a_plain_timer_slot():
    a, b, c = ac.case_reply_to_plain_timer_slot(make, 4)
    assert a["slots"][ac.ACTOR][4][1] == 1 and b["slots"][ac.ACTOR][4][1] == 129  # the same generation mod 2^7
    assert b["slots"][ac.ACTOR][0][1] == 1 and b["slots"][ac.ACTOR][5][1] == 0   # active, a plain timer's
    assert ac.echoes(c) == [] and c["info"] == dict(asked=1, answered=0, timed_out=0, late=1)


def test_generations_alias_mod_128():
    """bounded difference 4"""
    a, b, c = ac.case_generation_alias(make, 4)
    assert b["slots"][ac.ACTOR][4][0] == 129 and b["info"]["asked"] == 129
    assert ac.echoes(c) == [P("Adapted:6")] and c["info"] == dict(asked=129, answered=1, timed_out=0, late=0)


def test_ask_pending():
    a, b, c = ac.case_ask_pending(make, 1)
    assert ac.echoes(a) == [P("IsPending:1")] and ac.echoes(b) == [P("Adapted:6")] and ac.echoes(c) == [P("IsPending:0")]


def test_asking_oneself():
    (s,) = ac.case_ask_self(make, 4)
    assert ac.echoes(s) == [P("Adapted:3")] and s["info"] == dict(asked=1, answered=1, timed_out=0, late=0)
    assert s["timer_info"]["ticks"] == 2


def test_reply_sees_sender_self():
    """bounded difference 5: the snitch echoes Pong(0xBAD) for a Pong whose sender is not itself"""
    got = ac.run_kat("succeeds_while_alive", 4, make(ac.kat_workload("succeeds_while_alive", 4)))
    assert got["echo"] == [P("Pong:11")]


def test_dead_target_fails_after_the_timeout():
    """bounded difference 2: only the tick differs from the reference, which fails at once"""
    for name in ("target_already_terminated", "actor_does_not_exist"):
        got = ac.run_kat(name, 4, make(ac.kat_workload(name, 4)))
        assert got["echo"] == [P("TimedOut")] and got["ticks"] == 1 + 3


@pytest.mark.parametrize("name", ["same_bucket", "two_buckets", "all_ask", "pingpong_target", "timeout_only_bucket"])
def test_gpu_cases_on_the_model(name):
    snaps = ac.RULE_CASES[name](make, 4)
    s = snaps[-1]
    if name == "all_ask":
        assert s["info"] == dict(asked=80, answered=80, timed_out=0, late=0) and len(s["echo"][0]) == 80
    elif name == "timeout_only_bucket":
        assert s["info"] == dict(asked=1, answered=0, timed_out=1, late=0) and s["echo"][2] == [P("TimedOut")]
    elif name == "pingpong_target":
        assert ac.echoes(s) == [P("Pong:5")] and s["info"]["answered"] == 1
    else:
        assert ac.echoes(s) == [P("Adapted:5")] and s["info"]["answered"] == 1


def test_without_ask_it_is_the_timer_model():
    w = wl.heartbeat(64, period=4, n_host=2, bucket_actors=32)
    a, t = AskModel(**w.engine_kwargs()), TimerModel(**w.engine_kwargs())
    w.apply_to(a), w.apply_to(t)
    assert a.run(20) == t.run(20) and np.array_equal(a.read_state()[0], t.read_state()[0])


@pytest.mark.parametrize("wname", ["ask_pool", "ask_retry"])
def test_workloads(wname):
    if wname == "ask_pool":
        w = wl.ask_pool(96, 32, timeout=4, silent_every=4, period=8, bucket_actors=32)
        m = make(w)
        st = m.run(40)
        words, _ = m.read_state()
        info = m.ask_info()
        assert info["asked"] > 96 * 3 and info["late"] == 0
        assert int((words[:96, 0] & 0xFFFFFFFF).sum()) == info["answered"] and int((words[:96, 0] >> 32).sum()) == info["timed_out"]
        silent = np.arange(96) % 32 % 4 == 3
        assert (words[:96, 0][silent] & 0xFFFFFFFF).sum() == 0 and (words[:96, 0][~silent] >> 32).sum() == 0
    else:
        w = wl.ask_retry(64, 8, timeout=3, silent_every=2, bucket_actors=32)
        m = make(w)
        st = m.run()
        words, _ = m.read_state()
        info = m.ask_info()
        assert st["in_flight"] == 0 and info["answered"] + int((words[:64, 0] >> 32).sum()) == 64
        assert info["timed_out"] > 0 and info["answered"] > 0
    assert ac.conserved(ac.counts(st), m.timer_info())
