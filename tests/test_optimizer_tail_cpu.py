"""CPU: the bookkeeping of ops.TableGrad.slot / lookup (a lookup gradient whose second level is left to the optimizer's row
pass).  The library is replaced by a recorder, the stamps the first-level launch would write are written by hand: what is
checked is which launches the host issues in which order, and that no stamp and no recorded lookup outlives its gradient."""
import pytest
import torch

from util import pkg


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('srec_'):
            raise AttributeError(name)
        return lambda *a: self.calls.append(name)


@pytest.fixture
def tg(monkeypatch):
    ops = pkg('ops')
    rec = _Recorder()
    monkeypatch.setattr(ops, 'lib', rec)
    monkeypatch.setattr(ops, 'ptr', lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, 'stream', lambda: None)
    monkeypatch.delenv('SREC_LOOKUP_IN_ROWPASS', raising=False)
    W = torch.randn(20, 8)
    t = ops.TableGrad(W, defer=True)
    t.rec, t.W = rec, W
    return t


def _hand_over(t, rows=(0, 7, 19)):
    """what a two-level lookup backward does under a pending projection"""
    assert t.lookup_in_rowpass()
    for u, r in enumerate(rows):
        t.slot[r] = u + 1
    items = torch.tensor(list(rows), dtype=torch.int32)
    t.hand_over(torch.zeros(5, 8), torch.arange(len(rows) + 1, dtype=torch.int32), items, None)


def test_slot_exists_only_with_defer_and_the_switch_turns_the_deferral_off(tg, monkeypatch):
    ops = pkg('ops')
    assert ops.TableGrad(tg.W, defer=False).slot is None and not ops.TableGrad(tg.W, defer=False).lookup_in_rowpass()
    assert tg.slot.dtype == torch.int32 and tg.slot.shape == (20,) and int(tg.slot.abs().max()) == 0
    assert not tg.lookup_in_rowpass()                       # no pending projection: nothing to ride on
    tg.pending = (tg.W, torch.ones(20), 1.0)
    assert tg.lookup_in_rowpass()
    monkeypatch.setenv('SREC_LOOKUP_IN_ROWPASS', '0')
    assert not tg.lookup_in_rowpass()


def test_row_pass_takes_the_lookup_and_issues_no_fill(tg):
    tg.pending = (tg.W, torch.ones(20), 1.0)
    _hand_over(tg)
    assert tg.slot_dirty and tg.radial_dirty and tg.lookup is not None
    part = tg.take_lookup()[0]
    assert part.shape == (5, 8) and tg.lookup is None and not tg.slot_dirty
    assert tg.rec.calls == []                               # (the kernel clears the stamps: the host launches nothing)


def test_materialize_runs_the_second_level_then_projects_and_clears_the_stamps(tg):
    tg.pending = (tg.W, torch.ones(20), 1.0)
    _hand_over(tg)
    tg.materialize()
    assert tg.rec.calls == ['srec_scatter_add_sorted_ex', 'srec_rownorm_project_radial']
    assert tg.lookup is None and tg.pending is None and not tg.slot_dirty and int(tg.slot.abs().max()) == 0


@pytest.mark.parametrize('how', ['overwritten', 'reset'])
def test_overwritten_and_reset_drop_the_lookup_and_zero_a_dirty_slot(tg, how):
    tg.pending = (tg.W, torch.ones(20), 1.0)
    _hand_over(tg)
    tg.radial[3] = 2.0
    getattr(tg, how)()
    assert tg.rec.calls == []                               # dropped with the contents it belonged to, not flushed into them
    assert tg.lookup is None and tg.pending is None and not tg.slot_dirty and not tg.radial_dirty
    assert int(tg.slot.abs().max()) == 0 and float(tg.radial.abs().max()) == 0.0


def test_a_second_hand_over_needs_the_first_one_flushed(tg):
    tg.pending = (tg.W, torch.ones(20), 1.0)
    _hand_over(tg)
    with pytest.raises(AssertionError):
        _hand_over(tg, rows=(1, 2))
    tg.slot.zero_()
    for u, r in enumerate((0, 7, 19)):
        tg.slot[r] = u + 1
    tg.flush_lookup()                                       # what EmbeddingLookup.backward does first
    assert tg.rec.calls == ['srec_scatter_add_sorted_ex'] and int(tg.slot.abs().max()) == 0 and tg.pending is not None
    _hand_over(tg, rows=(1, 2))
    assert tg.lookup[2].tolist() == [1, 2]
