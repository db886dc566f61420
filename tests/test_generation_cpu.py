"""CPU: the replay driver of generate() and of the device beam search (generation._run_steps) with a counting step and no graph - how many steps run, and
when the `closed` predicate is consulted."""
import pytest

from audio_flamingo_amd.generation import _run_steps


def _drive(max_new, closes_at):
    steps, asked = [], []

    def closed(t):
        asked.append(t)
        return closes_at is not None and t >= closes_at

    n = _run_steps(lambda: steps.append(1), max_new, False, closed)
    assert n == len(steps)
    return n, asked


@pytest.mark.parametrize("max_new", [20, 33])
def test_run_steps_polls_every_eighth_step_in_front_of_it(max_new):
    polls = [t for t in range(1, max_new) if t % 8 == 0]
    n, asked = _drive(max_new, 8)
    assert n == 7 and asked == [8]
    n, asked = _drive(max_new, 16)
    assert n == 15 and asked == [8, 16]
    n, asked = _drive(max_new, None)
    assert n == max_new - 1 and asked == polls
    n, asked = _drive(max_new, 11)   # a rule that closes between two polls is seen at the next one: the steps up to it have run
    assert n == 15 and asked == [8, 16]


def test_run_steps_with_one_token_runs_nothing():
    assert _drive(1, None) == (0, [])
    assert _drive(1, 8) == (0, [])


def test_run_steps_calls_after_behind_every_step():
    order = []
    assert _run_steps(lambda: order.append("step"), 4, False, lambda t: False, after=lambda: order.append("after")) == 3
    assert order == ["step", "after"] * 3
