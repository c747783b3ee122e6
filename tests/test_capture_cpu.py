"""graph.Capture's pin bookkeeping and models.capture_generic_path, the parts that need no GPU: stand-in plans with a counting
pin(delta) are handed out through rspmm's plan recorder, as get_plan() hands out real ones."""
import threading

import pytest

from ultra_amd import models, rspmm
from ultra_amd.graph import Capture


class FakePlan(object):
    def __init__(self, exact=True):
        self.exact, self.pins, self.calls = exact, 0, 0

    def pin(self, delta=1):
        self.pins += delta
        self.calls += 1


def ask_for(*plans):
    """What rspmm.get_plan does for a recording capture."""
    for plan in plans:
        rspmm._PLAN_RECORDER.append(plan)


def test_each_distinct_plan_of_the_warm_up_is_pinned_once_and_release_is_idempotent():
    a, b = FakePlan(), FakePlan()
    capture = Capture(None)
    assert capture.plans == [] and capture.exact_order
    with capture.recording():
        ask_for(a, b, a, a)
        assert (a.pins, b.pins) == (0, 0)          # (pinned when the warm-up is over: exactly what it asked for)
        ask_for(b)
    assert (a.pins, b.pins) == (1, 1) and (a.calls, b.calls) == (1, 1)
    assert capture.plans == [a, b] and capture.exact_order
    capture.release()
    capture.release()
    assert (a.pins, b.pins) == (0, 0) and (a.calls, b.calls) == (2, 2)
    assert capture.plans == [] and capture.graphs == []


def test_exact_order_speaks_of_the_plans_the_capture_uses():
    capture = Capture(None)
    with capture.recording():
        ask_for(FakePlan(), FakePlan(exact=False))
    assert not capture.exact_order


def test_a_second_warm_up_lets_go_of_the_plans_of_the_first():
    a, b = FakePlan(), FakePlan()
    capture = Capture(None)
    with capture.recording():
        ask_for(a, b)
    with capture.recording():
        ask_for(b)
    assert (a.pins, b.pins) == (0, 1) and capture.plans == [b]
    del capture                                     # (the only reference: __del__ releases)
    assert (a.pins, b.pins) == (0, 0)


@pytest.mark.parametrize("error", [RuntimeError, KeyboardInterrupt])
def test_an_exception_inside_the_warm_up_leaves_nothing_pinned(error):
    a, b = FakePlan(), FakePlan()
    capture = Capture(None)
    with capture.recording():
        ask_for(a)
    outer = rspmm._PLAN_RECORDER
    with pytest.raises(error):
        with capture.recording():
            ask_for(a, b)
            raise error("warm-up failed")
    assert (a.pins, b.pins) == (0, 0) and capture.plans == []
    assert rspmm._PLAN_RECORDER is outer


def test_a_pin_that_fails_unpins_the_plans_pinned_before_it():
    class Refusing(FakePlan):
        def pin(self, delta=1):
            raise RuntimeError("pin refused")
    a = FakePlan()
    capture = Capture(None)
    with pytest.raises(RuntimeError, match="pin refused"):
        with capture.recording():
            ask_for(a, Refusing())
    assert a.pins == 0 and a.calls == 2 and capture.plans == []


def test_a_nested_recording_still_hands_its_plans_to_the_outer_one():
    a, b, c = FakePlan(), FakePlan(), FakePlan()
    capture = Capture(None)
    assert rspmm._PLAN_RECORDER is None
    with rspmm.record_plans() as outer:
        ask_for(c)
        with capture.recording():
            ask_for(a, b, a)
    assert rspmm._PLAN_RECORDER is None
    assert outer.plans == [c, a, b]
    assert capture.plans == [a, b] and (a.pins, b.pins, c.pins) == (1, 1, 0)


def test_the_generic_path_flag_is_scoped_to_its_block_and_its_thread():
    assert not models.generic_path_capturable()
    seen = {}

    def elsewhere():
        seen["other thread"] = models.generic_path_capturable()
    with models.capture_generic_path():
        assert models.generic_path_capturable()
        thread = threading.Thread(target=elsewhere)
        thread.start()
        thread.join()
    assert seen == {"other thread": False}
    assert not models.generic_path_capturable()
    with pytest.raises(RuntimeError, match="inside"):
        with models.capture_generic_path():
            raise RuntimeError("inside")
    assert not models.generic_path_capturable()
