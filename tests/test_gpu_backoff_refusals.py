"""The refusals of restartWithBackoff (agx_set_backoff), each with its status and text, in both call
orders where there are two; afterwards the engine still runs and equals an engine that never saw the refused call."""
import ctypes

import pytest

from akka_amd import typed
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine
from tests import backoff_cases as bc

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 6
NAME, T = "restart_after_exponential_backoff", 3
NO_SUPERVISION = "backoff needs an engine with supervision (agx_set_supervision first)"


def status_and_text(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]   # ("AGX_EINVAL: <the engine's text>")


def bare(w, supervision=True):
    """an engine with the workload's actors and tables and, unless told otherwise, its supervision; backoff not set"""
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    for first, count, kind, init in w.ranges:
        eng.register_range(first, count, kind, init)
    eng.set_outbound(*w.outbound)
    eng.set_behaviors(w.behaviors)
    if supervision:
        eng.set_supervision(w.supervision["rows"])
    return eng


def finish(eng):
    got = bc.run_kat(NAME, T, eng)
    eng.close()
    return got


def row(**kw):
    return typed.AgxBackoff(**dict(dict(min_backoff=4, max_backoff=40, random_factor_q16=0, reset_after=40, stash_capacity=0), **kw))


def raw(eng, rows, n_behaviors, n_levels):
    """agx_set_backoff with dimensions of the caller's choosing"""
    from akka_amd._lib import check
    arr = (typed.AgxBackoff * max(len(rows), 1))(*rows)
    check(eng.lib.agx_set_backoff(eng._h, ctypes.cast(arr, ctypes.c_void_p), n_behaviors, n_levels))


@pytest.fixture(scope="module")
def untouched(built):
    """the script on an engine that never saw a refused call"""
    w = bc.kat_workload(NAME, T)
    eng = bare(w)
    eng.set_backoff(w.supervision["backoff"])
    got = finish(eng)
    bc.check_kat(NAME, T, got)
    return got


def test_before_supervision(built, untouched):
    w = bc.kat_workload(NAME, T)
    eng = bare(w, supervision=False)
    assert status_and_text(lambda: eng.set_backoff(w.supervision["backoff"])) == (EINVAL, NO_SUPERVISION)
    eng.set_supervision(w.supervision["rows"])
    eng.set_backoff(w.supervision["backoff"])
    assert finish(eng) == untouched


def test_second_call(built, untouched):
    w = bc.kat_workload(NAME, T)
    eng = bare(w)
    eng.set_backoff(w.supervision["backoff"])
    assert status_and_text(lambda: eng.set_backoff(w.supervision["backoff"])) == \
        (EINVAL, "backoff is set once (agx_set_supervision with another table drops the rows)")
    assert finish(eng) == untouched


def test_after_the_first_run(built):
    w = bc.kat_workload(NAME, T)
    eng = bare(w)
    eng.run()
    assert status_and_text(lambda: eng.set_backoff(w.supervision["backoff"])) == (ESTATE, "set backoff before the first agx_run")
    assert eng.backoff_info() == dict(backoffs=0, resumed=0, dropped=0, limit_stops=0, suspended=0)
    eng.close()


def test_dimensions(built, untouched):
    w = bc.kat_workload(NAME, T)
    eng = bare(w)
    text = "backoff: %u levels for %u behaviours; agx_set_supervision had 1 levels for 1 behaviours"
    assert status_and_text(lambda: raw(eng, [row(), row()], 1, 2)) == (EINVAL, text.replace("%u", "2", 1).replace("%u", "1", 1))
    assert status_and_text(lambda: raw(eng, [row(), row()], 2, 1)) == (EINVAL, text.replace("%u", "1", 1).replace("%u", "2", 1))
    eng.set_backoff(w.supervision["backoff"])
    assert finish(eng) == untouched


@pytest.mark.parametrize("bad", [dict(min_backoff=5, max_backoff=4), dict(max_backoff=1 << 31), dict(random_factor_q16=65537),
                                 dict(reset_after=0), dict(stash_capacity=-2)])
def test_bad_row(built, untouched, bad):
    w = bc.kat_workload(NAME, T)
    eng = bare(w)
    assert status_and_text(lambda: eng.set_backoff([[row(**bad)]])) == \
        (EINVAL, "backoff: bad row 0 of behaviour 0 (1 <= min_backoff <= max_backoff <= 2^31 - 1 ticks, random_factor_q16 <= "
                 "65536, reset_after >= 1 tick, stash_capacity >= -1)")
    eng.set_backoff(w.supervision["backoff"])
    assert finish(eng) == untouched


@pytest.mark.parametrize("entry", ["resume", "stop", "unused"])
def test_row_on_an_entry_that_does_not_restart(built, entry):
    excs = bc.sc.exception_types(bc.KATS["classes"])
    sup = [["Exc1", "restart"]] if entry == "unused" else [["Exc1", entry], ["Exc3", "restart"]]
    b = bc.target_behavior(sup, excs)
    tb = typed.compile_behaviors([b], max_emit=1)
    w = bc.workload_of(tb, "refusal", bc.N_KAT, T, tb.kind_of(b))
    eng = bare(w)
    text = "backoff: row %d of behaviour 0 stands on an entry that is not AGX_SUP_RESTART"
    if entry == "unused":   # two levels, the second entry unused (class_mask 0)
        eng.set_supervision([list(tb.supervisors[0]) + [typed.AgxSupervisor()]])
        assert status_and_text(lambda: eng.set_backoff([[row(), row()]])) == (EINVAL, text % 1)
        eng.set_backoff([[row(), typed.AgxBackoff()]])
    else:
        assert status_and_text(lambda: eng.set_backoff([[row(), row()]])) == (EINVAL, text % 0)
        eng.set_backoff([[typed.AgxBackoff(), row()]])
    eng.close()


def test_inherits_the_supervision_engines_refusals(built, untouched):
    """the features supervision shares no engine with, in both call orders"""
    w = bc.kat_workload(NAME, T)
    eng = bare(w)
    eng.set_backoff(w.supervision["backoff"])
    for call in (lambda: eng.set_timers(1), lambda: eng.set_death_watch(1), lambda: eng.set_receptionist(1, 8)):
        st, text = status_and_text(call)
        assert st == EINVAL and "supervision (agx_set_supervision)" in text
    assert finish(eng) == untouched
    for first in ("set_timers", "set_death_watch"):
        eng = bare(w, supervision=False)
        getattr(eng, first)(1)
        assert status_and_text(lambda: eng.set_supervision(w.supervision["rows"]))[0] == EINVAL
        assert status_and_text(lambda: eng.set_backoff(w.supervision["backoff"])) == (EINVAL, NO_SUPERVISION)
        eng.close()
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), max_emit=2)))
    assert status_and_text(lambda: eng.set_supervision(w.supervision["rows"]))[0] == EINVAL
    assert status_and_text(lambda: eng.set_backoff(w.supervision["backoff"])) == (EINVAL, NO_SUPERVISION)
    eng.close()


def test_another_supervision_table_drops_the_rows(built, untouched):
    w = bc.kat_workload(NAME, T)
    eng = bare(w)
    eng.set_backoff(w.supervision["backoff"])
    eng.set_supervision(w.supervision["rows"])      # the same table: the rows stay
    assert status_and_text(lambda: eng.set_backoff(w.supervision["backoff"]))[0] == EINVAL
    other = typed.AgxSupervisor.from_buffer_copy(bytes(w.supervision["rows"][0][0]))
    other.max_restarts = 7
    eng.set_supervision([[other]])                  # another one: they are dropped, and can be set again
    eng.set_supervision(w.supervision["rows"])
    eng.set_backoff(w.supervision["backoff"])
    assert finish(eng) == untouched
