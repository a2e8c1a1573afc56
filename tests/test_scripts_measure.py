"""CPU: the rules of scripts/measure.py that every speed claim under profiles/ rests on -- the every-window verdict, the
order in which paths alternate, the endless batch stream, the window statistics, and the refusal to run without a GPU."""
import pytest

from scripts import measure


# -- the every-window rule -------------------------------------------------------------------------------------------------
WIN = [1.0, 1.5, 2.0]
CASES = [                                     # (a, b, a wins, b wins)
    (WIN, [2.5, 3.0, 2.1], True, False),      # clear win: max(a) = 2.0 < min(b) = 2.1
    ([2.5, 3.0, 2.1], WIN, False, True),      # clear loss
    (WIN, [1.2, 1.7, 2.2], False, False),     # interleaved windows
    (WIN, [2.0, 2.5, 3.0], False, False),     # the tie max(a) == min(b) is an overlap
    ([2.0, 2.5, 3.0], WIN, False, False),     # ... from either side
]


@pytest.mark.parametrize('a,b,a_wins,b_wins', CASES)
def test_verdict_claims_shorter_only_under_strict_inequality(a, b, a_wins, b_wins):
    assert measure.every_window_shorter(a, b) is a_wins
    assert measure.every_window_shorter(b, a) is b_wins
    want = 'step faster' if a_wins else ('module faster' if b_wins else 'within the spread')
    assert measure.verdict(a, b, 'step', 'module') == want
    want = ('every grouped window is shorter than every per-tensor window' if a_wins else
            'every per-tensor window is shorter than every grouped window' if b_wins else 'the windows overlap')
    assert measure.verdict(a, b, 'grouped', 'per-tensor', style='windows') == want


def test_verdict_refuses_an_unknown_style():
    with pytest.raises(AssertionError):
        measure.verdict(WIN, WIN, 'a', 'b', style='loose')


# -- alternation -----------------------------------------------------------------------------------------------------------
def test_alternate_is_round_major_in_dict_order_with_before_ahead_of_each_window():
    log = []
    fns = {name: (lambda name=name: name) for name in ('engine', 'phases', 'module')}      # (not in sorted order)

    def window(fn):
        log.append(('window', fn()))
        return len(log)

    got = measure.alternate(fns, window, 4, before=lambda name: log.append(('before', name)))
    want = []
    for _ in range(4):
        for name in ('engine', 'phases', 'module'):
            want += [('before', name), ('window', name)]
    assert log == want
    assert list(got) == ['engine', 'phases', 'module']
    assert all(len(v) == 4 for v in got.values())
    # a path's values are its own windows', in round order: window k of the log (1-based, two entries per window)
    assert got == {'engine': [2, 8, 14, 20], 'phases': [4, 10, 16, 22], 'module': [6, 12, 18, 24]}


def test_alternate_without_before_calls_only_the_windows():
    calls = []
    got = measure.alternate({'a': 'A', 'b': 'B'}, lambda fn: calls.append(fn) or fn.lower(), 2)
    assert calls == ['A', 'B', 'A', 'B'] and got == {'a': ['a', 'a'], 'b': ['b', 'b']}


def test_split_counts_separates_times_from_launches():
    ms, launches = measure.split_counts({'a': [(1.0, 7.0), (2.0, 7.5)], 'b': [(3.0, 9.0)]})
    assert ms == {'a': [1.0, 2.0], 'b': [3.0]} and launches == {'a': [7.0, 7.5], 'b': [9.0]}


# -- cycle -----------------------------------------------------------------------------------------------------------------
class Epochs(object):
    """An iterable that, like ClusterIter, is exhausted after one pass and starts a new one when iterated again."""

    def __init__(self):
        self.passes = 0

    def __iter__(self):
        self.passes += 1
        return iter([(self.passes, k) for k in range(3)])


def test_cycle_restarts_an_exhausted_iterable_and_yields_every_element_of_each_pass():
    it = Epochs()
    stream = measure.cycle(it)
    got = [next(stream) for _ in range(8)]
    assert got == [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1)]
    assert it.passes == 3


# -- statistics ------------------------------------------------------------------------------------------------------------
def test_stats_spread_and_cell_on_a_hand_computed_list():
    ws = [1.23456, 1.11114, 1.99996, 1.50004]             # sorted: 1.11114 1.23456 1.50004 1.99996; median 1.3673
    assert measure.stats(ws) == dict(median=1.3673, min=1.1111, max=2.0, windows=[1.2346, 1.1111, 2.0, 1.5])
    assert measure.summary(ws) == (pytest.approx(1.3673, rel=1e-15), 1.11114, 1.99996)
    assert measure.spread(ws) == pytest.approx(0.88882 / 1.3673, rel=1e-12)
    assert measure.cell(ws) == '1.367 (1.111 .. 2.000)'
    assert measure.cell([10.04, 30.06, 20.06], 1) == '20.1 (10.0 .. 30.1)'
    odd = [3.0, 1.0, 2.0]
    assert measure.stats(odd)['median'] == 2.0 and measure.spread(odd) == 1.0


# -- no fallback -----------------------------------------------------------------------------------------------------------
def test_require_gpu_exits_without_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit) as e:
        measure.require_gpu('some_tool.py')
    assert 'some_tool.py measures on the GPU' in str(e.value) and e.value.code != 0
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    assert measure.require_gpu('some_tool.py') is None
