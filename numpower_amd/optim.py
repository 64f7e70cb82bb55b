"""Stateful optimizers over NDArray.dnn_sgd_step / dnn_adam_step / dnn_grad_norm: SGD, Adam and AdamW with torch's
keyword names.  An optimizer holds the list of parameters (GPU arrays, updated in place), owns zero-initialised state arrays on the
same device and the step count, and updates the whole list in one launch per 64 tensors.

    opt = optim.AdamW(params, lr=1e-3, weight_decay=1e-2)
    opt.step(grads, max_norm=1.0)       # clip_grad_norm_(max_norm) and the update, with no host read in between
    opt.last_norm                       # the (2) GPU array (norm, coefficient) of that call

Not here: parameter groups, amsgrad, maximize, learning-rate schedules and state dictionaries."""
from __future__ import annotations

from .ndarray import GPU, Error, NDArray

__all__ = ["SGD", "Adam", "AdamW"]


def _number(who, name, value):
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise Error("%s: %s must be a number" % (who, name))
    return float(value)


class _Optimizer:
    def __init__(self, params):
        who = type(self).__name__
        if not isinstance(params, (list, tuple)) or not params or any(not isinstance(p, NDArray) for p in params):
            raise Error(who + ": params must be a non-empty list of arrays")
        self.params = list(params)
        self.steps = 0
        self.last_norm = None

    def _zeros(self):
        return [NDArray.zeros(p.shape(), GPU) for p in self.params]

    def _clip(self, grads, max_norm):
        """-> grad_scale for the step: None, or (last_norm, 1) after the list's norm has been taken"""
        who = type(self).__name__
        if not isinstance(grads, (list, tuple)) or len(grads) != len(self.params):
            raise Error(who + ".step: grads must be a list with one gradient per parameter")
        if max_norm is None:
            return None
        self.last_norm = NDArray.dnn_grad_norm(grads, _number(who + ".step", "max_norm", max_norm))
        return (self.last_norm, 1)


class SGD(_Optimizer):
    """torch.optim.SGD: lr, momentum, dampening, weight_decay, nesterov"""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        super().__init__(params)
        self.lr, self.momentum, self.dampening, self.weight_decay = (_number("SGD", n, v) for n, v in (
            ("lr", lr), ("momentum", momentum), ("dampening", dampening), ("weight_decay", weight_decay)))
        self.nesterov = bool(nesterov)
        if self.lr < 0.0 or self.weight_decay < 0.0 or not 0.0 <= self.momentum <= 1.0 or not 0.0 <= self.dampening <= 1.0:
            raise Error("SGD: lr and weight_decay must not be negative, momentum and dampening must lie in [0, 1]")
        if self.nesterov and (self.momentum == 0.0 or self.dampening != 0.0):
            raise Error("SGD: nesterov needs a momentum and zero dampening")
        self.buffers = self._zeros() if self.momentum != 0.0 else None

    def step(self, grads, max_norm=None):
        scale = self._clip(grads, max_norm)
        NDArray.dnn_sgd_step(self.params, list(grads), self.lr, self.momentum, self.dampening, self.weight_decay, self.nesterov, self.buffers,
                             first_step=self.steps == 0, grad_scale=scale)
        self.steps += 1


class Adam(_Optimizer):
    """torch.optim.Adam: lr, betas, eps, weight_decay (L2: it joins the gradient)"""
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params)
        who = type(self).__name__
        if not isinstance(betas, (tuple, list)) or len(betas) != 2:
            raise Error(who + ": betas must be a pair of numbers")
        self.lr, self.eps, self.weight_decay = (_number(who, n, v) for n, v in (("lr", lr), ("eps", eps), ("weight_decay", weight_decay)))
        self.betas = (_number(who, "betas", betas[0]), _number(who, "betas", betas[1]))
        if self.lr < 0.0 or self.eps < 0.0 or self.weight_decay < 0.0 or not all(0.0 <= b < 1.0 for b in self.betas):
            raise Error(who + ": lr, eps and weight_decay must not be negative, the betas must lie in [0, 1)")
        self.exp_avg, self.exp_avg_sq = self._zeros(), self._zeros()

    def step(self, grads, max_norm=None):
        scale = self._clip(grads, max_norm)
        NDArray.dnn_adam_step(self.params, list(grads), self.exp_avg, self.exp_avg_sq, self.steps + 1, self.lr, self.betas, self.eps,
                              self.weight_decay, self._decoupled, scale)
        self.steps += 1


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay, p = p - lr . weight_decay . p before the update"""
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr, betas, eps, weight_decay)
