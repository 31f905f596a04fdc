"""The epoch loop MLPCONV.fit and RowPartitionedMLPCONV.fit share (mlpconv.fit_loop), with
scripted steps and CPU tensors as the parameters: validation every report_k_epoch, strict `<`
on the dev loss, early stopping, the best-parameter restore and the final dev evaluation of
mlpconv.py:290-318. Then the loop under it that the mini-batch trainers run too
(training.run_epochs) with their improvement rules, the abort predicate and the per-epoch hook,
and the host half of the two optimisers. No kernel runs."""
import math

import numpy as np
import pytest
import torch

from graphconvgeo_amd import training as T
from graphconvgeo_amd.dist_train import RowPartitionedMLPCONV
from graphconvgeo_amd.loc2lang import LasagneAdamax
from graphconvgeo_amd.mlpconv import MLPCONV, LasagneAdam, fit_loop

DEV_LOSS = {0: 3.0, 2: 2.0, 4: 2.5, 6: 2.5, 8: 1.0}


class Script:
    """train_step writes the epoch number into the parameters; evaluate reads the dev loss of
    the last epoch trained and records what the parameters held when it was called."""

    def __init__(self):
        self.params = [torch.zeros(3), torch.zeros(2, 2)]
        self.epoch = -1
        self.evaluated = []  # (epoch, value of the parameters) per evaluate() call

    def train_step(self):
        self.epoch += 1
        with torch.no_grad():
            for p in self.params:
                p.fill_(float(self.epoch))
        return torch.tensor(10.0 - self.epoch), torch.tensor(0.1 * self.epoch)

    def evaluate(self):
        self.evaluated.append((self.epoch, float(self.params[0][0])))
        return torch.tensor(DEV_LOSS[self.epoch]), torch.tensor(0.01 * self.epoch)


def test_loop_validates_stops_restores_and_evaluates_once_more():
    s, history = Script(), []
    final = fit_loop(s.train_step, s.evaluate, s.params, history, n_epochs=10, report_k_epoch=2,
                     early_stopping_max_down=1)
    # epoch 4: n_down = 1, not > 1; epoch 6: n_down = 2 > 1 -- the loop stops after epoch 6
    assert s.epoch == 6
    assert [r["epoch"] for r in history] == list(range(7))
    for r in history:
        assert ("val_loss" in r and "val_acc" in r) == (r["epoch"] % 2 == 0)
        assert r["train_loss"] == 10.0 - r["epoch"]
        assert r["train_acc"] == pytest.approx(0.1 * r["epoch"])
    assert [history[n]["val_loss"] for n in (0, 2, 4, 6)] == [3.0, 2.0, 2.5, 2.5]
    # the parameters snapshotted at epoch 2 (the lowest dev loss) are back
    for p in s.params:
        assert torch.equal(p, torch.full_like(p, 2.0))
    # four validations, then exactly one more evaluation, after the restore
    assert [e for e, _ in s.evaluated] == [0, 2, 4, 6, 6]
    assert s.evaluated[-1][1] == 2.0 and s.evaluated[-2][1] == 6.0
    assert final == (2.5, pytest.approx(0.06))  # evaluate() as scripted for the last epoch


def test_equal_dev_loss_is_not_an_improvement():
    s, history = Script(), []
    fit_loop(s.train_step, s.evaluate, s.params, history, n_epochs=7, report_k_epoch=2,
             early_stopping_max_down=100)
    # 2.5 at epoch 6 does not beat 2.0 at epoch 2 (nor equal 2.5 at epoch 4)
    assert s.epoch == 6 and all(float(p.flatten()[0]) == 2.0 for p in s.params)


def test_no_epochs_restores_nothing_and_still_evaluates():
    s, history = Script(), []
    s.epoch = 0  # evaluate() reads DEV_LOSS[0]
    for p in s.params:
        p.fill_(7.0)
    final = fit_loop(s.train_step, s.evaluate, s.params, history, n_epochs=0, report_k_epoch=2,
                     early_stopping_max_down=1)
    assert history == [] and s.evaluated == [(0, 7.0)]
    assert all(torch.equal(p, torch.full_like(p, 7.0)) for p in s.params)
    assert final == (3.0, 0.0)


@pytest.mark.parametrize("bad", [dict(dtype="float64"), dict(complete_prob=True),
                                 dict(loss_name="hinge"), dict(order="x")])
def test_both_trainers_refuse_the_same_arguments(bad):
    raised = []
    for make in (lambda: MLPCONV(device="cpu", **bad),
                 lambda: RowPartitionedMLPCONV(device="cpu", rank=0, world=1, **bad)):
        with pytest.raises((ValueError, NotImplementedError)) as e:
            make()
        raised.append(e.type)
    assert raised[0] is raised[1]


# -- the loop of the mini-batch trainers: one scripted case per rule -----------------------------
class Epochs:
    """train_epoch(n) writes n + 1 into the parameters; evaluate() returns the scripted dev
    figures of the last epoch trained. Every call is noted in `calls`."""

    def __init__(self, dev):
        self.params = [torch.zeros(3), torch.zeros(2, 2)]
        self.dev, self.calls, self.epoch = dev, [], -1

    def train_epoch(self, n):
        self.epoch = n
        self.calls.append(("train", n))
        with torch.no_grad():
            for p in self.params:
                p.fill_(float(n + 1))
        return (torch.tensor(10.0 - n),) + ((torch.tensor(0.5),) if len(self.dev[n]) == 2 else ())

    def evaluate(self):
        self.calls.append(("evaluate", self.epoch))
        return tuple(torch.tensor(x, dtype=torch.float64) for x in self.dev[self.epoch])

    def hook(self, n):
        self.calls.append(("hook", n))

    def run(self, improved, max_down=100, **kw):
        history = []
        out = T.run_epochs(self.train_epoch, self.evaluate, self.params, history, len(self.dev),
                           improved, max_down, **kw)
        return out, history

    def holds(self, value):
        return all(torch.equal(p, torch.full_like(p, float(value))) for p in self.params)


def test_accuracy_rule_equal_accuracy_is_not_an_improvement():
    s = Epochs([(3.0, 0.25), (1.0, 0.25), (2.0, 0.5), (0.5, 0.5)])
    (best, snap), history = s.run(T.higher_accuracy)
    # epoch 1 (lower loss, equal accuracy) and epoch 3 (equal again) are down steps
    assert best == (2.0, 0.5) and all(torch.equal(b, torch.full_like(b, 3.0)) for b in snap)
    assert [r["val_acc"] for r in history] == [0.25, 0.25, 0.5, 0.5]
    assert list(history[0]) == ["epoch", "train_loss", "train_acc", "val_loss", "val_acc"]
    T.restore(s.params, snap)
    assert s.holds(3.0)
    # the two down steps are not consecutive, yet both count: the counter restarts at a snapshot
    s = Epochs([(3.0, 0.25), (1.0, 0.25), (1.0, 0.25), (2.0, 0.5)])
    _, history = s.run(T.higher_accuracy, max_down=1)
    assert len(history) == 3


def test_accuracy_rule_never_above_zero_snapshots_nothing():
    s = Epochs([(3.0, 0.0), (2.0, 0.0), (1.0, 0.0)])
    (best, snap), history = s.run(T.higher_accuracy)
    assert snap is None and best == (math.inf, 0.0) and len(history) == 3
    T.restore(s.params, snap)
    assert s.holds(3.0)  # the last epoch's parameters stay


def test_relative_margin_rule():
    # 1.0 -> 0.99995: lower, but by 5e-5 < 1e-4 * 0.99995: a down step. 1.0 -> 0.9998: by 2e-4,
    # over the margin: a snapshot. Then 0.9998 -> 0.99975: lower by 5e-5 only, down again.
    s = Epochs([(1.0,), (0.99995,), (0.9998,), (0.99975,)])
    (best, snap), history = s.run(T.lower_loss_by_margin)
    assert best == (0.9998,) and all(torch.equal(b, torch.full_like(b, 3.0)) for b in snap)
    assert [r["val_loss"] for r in history] == [1.0, 0.99995, 0.9998, 0.99975]
    assert list(history[0]) == ["epoch", "train_loss", "val_loss"]  # no accuracy, no such keys
    # the same figures under the plain rule: every one of them is an improvement
    s = Epochs([(1.0,), (0.99995,), (0.9998,), (0.99975,)])
    (best, snap), _ = s.run(T.lower_loss)
    assert best == (0.99975,) and all(torch.equal(b, torch.full_like(b, 4.0)) for b in snap)
    # with one down step allowed, the second one in a row stops the loop
    s = Epochs([(1.0,), (0.99995,), (0.99991,), (0.5,)])
    _, history = s.run(T.lower_loss_by_margin, max_down=1)
    assert len(history) == 3


def test_rules_are_strict_and_written_on_the_new_loss():
    assert not T.lower_loss((2.0,), (2.0,)) and T.lower_loss((1.0,), (math.inf, 0.0))
    assert not T.higher_accuracy((0.0, 0.5), (9.0, 0.5))
    assert not T.higher_accuracy((0.0, 0.0), (math.inf, 0.0))
    # best - l_val > 0.0001 * l_val: 0.5 * 2^-12 on either side of 1e-4 * 0.5
    assert T.lower_loss_by_margin((0.5,), (0.5 + 2.0 ** -14,))
    assert not T.lower_loss_by_margin((0.5,), (0.5 + 2.0 ** -15,))
    assert not T.lower_loss_by_margin((float("nan"),), (math.inf, 0.0))
    assert T.lower_loss_by_margin((1e30,), (math.inf, 0.0))


def test_abort_in_the_first_epoch_leaves_history_empty_and_the_parameters_alone():
    s = Epochs([(float("nan"),), (1.0,)])
    out, history = s.run(T.lower_loss, abort=np.isnan, after_epoch=s.hook)
    assert out is None and history == []
    assert s.calls == [("train", 0), ("evaluate", 0)]  # nothing after the NaN
    assert s.holds(1.0)  # what epoch 0 trained: no snapshot was copied over it


def test_abort_in_a_later_epoch_keeps_the_earlier_records_and_skips_the_restore():
    s = Epochs([(2.0,), (3.0,), (float("nan"),), (1.0,)])
    out, history = s.run(T.lower_loss, abort=np.isnan)
    assert out is None
    assert [(r["epoch"], r["val_loss"]) for r in history] == [(0, 2.0), (1, 3.0)]
    assert s.holds(3.0)  # epoch 2's parameters, not the snapshot of epoch 0
    # without the predicate a NaN is a down step like any other
    s = Epochs([(2.0,), (float("nan"),), (1.0,)])
    (best, _), history = s.run(T.lower_loss)
    assert best == (1.0,) and len(history) == 3


def test_hook_runs_once_per_epoch_after_its_validation():
    s = Epochs([(2.0,), (3.0,), (1.0,)])
    s.run(T.lower_loss, after_epoch=s.hook)
    assert s.calls == [(what, n) for n in range(3) for what in ("train", "evaluate", "hook")]


# -- the optimisers' host half ---------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


@pytest.mark.parametrize("cls,key,a_t", [
    (LasagneAdam, "v", lambda lr, b1, b2, t: lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)),
    (LasagneAdamax, "u", lambda lr, b1, b2, t: lr / (1 - b1 ** t))])
def test_optimizer_step_size_and_state_round_trip(cls, key, a_t):
    ps = [torch.zeros(3), torch.zeros(2, 2)]
    lr, b1, b2 = 0.003, 0.8, 0.99
    opt = cls(ps, lr=lr, beta1=b1, beta2=b2)
    for t in (1, 2, 3):
        opt.prepare()
        assert opt.t == t and opt.a_t.dtype == torch.float32
        assert float(opt.a_t) == f32(a_t(lr, b1, b2, t))  # rounded once, from the double
    assert cls(ps).lr == {"v": 4e-3, "u": 2e-3}[key]  # the default learning rates stay
    second = getattr(opt, key)
    for i, (m, s) in enumerate(zip(opt.m, second)):
        m.fill_(1.0 + i)
        s.fill_(10.0 + i)
    st = opt.state()
    assert sorted(st) == sorted(["t", "m", key]) and st["t"] == 3
    opt.m[0].zero_()  # the state holds copies
    assert float(st["m"][0][0]) == 1.0
    other = cls(ps)
    other.load_state(st)
    assert other.t == 3
    for i in range(2):
        assert torch.equal(other.m[i], torch.full_like(ps[i], 1.0 + i))
        assert torch.equal(getattr(other, key)[i], torch.full_like(ps[i], 10.0 + i))
