"""The schedules of the reference's training step, restated as plain functions of the step (no torch, no state on the
device): the host knows the step, so the kernels take lr, beta1 and the loss weights as arguments.

``one_cycle``: torch.optim.lr_scheduler.OneCycleLR as configure_optimizers leaves it (networks/task/forced_alignment.py
:487-497: only max_lr and total_steps are passed) -- pct_start 0.3, cosine annealing, div_factor 25, final_div_factor
1e4, two phases, and cycle_momentum, which moves AdamW's beta1 between 0.95 and 0.85 against the learning rate.
``GaussianRampUp`` / ``NoneScheduler``: networks/scheduler/gaussian_ramp_up_scheduler.py:4-35, the per-loss weights of
forced_alignment.py:70-79.
"""
from __future__ import annotations

import math

PCT_START, DIV_FACTOR, FINAL_DIV_FACTOR = 0.3, 25.0, 1e4
BASE_MOMENTUM, MAX_MOMENTUM = 0.85, 0.95


def _cos(start, end, pct):
    """OneCycleLR._annealing_cos."""
    cos_out = math.cos(math.pi * pct) + 1
    return end + (start - end) / 2.0 * cos_out


def one_cycle(step: int, total_steps: int, max_lr: float):
    """(lr, beta1) of the optimiser step number ``step`` (0-based: the values OneCycleLR has set when that
    optimizer.step() runs).  ValueError past total_steps, as torch raises."""
    step, total_steps = int(step), int(total_steps)
    if total_steps <= 0:
        raise ValueError("one_cycle: total_steps must be positive")
    if not 0 <= step < total_steps:
        raise ValueError(f"one_cycle: step {step} is outside 0..{total_steps - 1}")
    initial_lr = max_lr / DIV_FACTOR
    min_lr = initial_lr / FINAL_DIV_FACTOR
    phases = ((float(PCT_START * total_steps) - 1, initial_lr, max_lr, MAX_MOMENTUM, BASE_MOMENTUM),
              (total_steps - 1, max_lr, min_lr, BASE_MOMENTUM, MAX_MOMENTUM))
    start_step = 0.0
    for i, (end_step, lr0, lr1, m0, m1) in enumerate(phases):
        if step <= end_step or i == len(phases) - 1:
            pct = (step - start_step) / (end_step - start_step)
            return _cos(lr0, lr1, pct), _cos(m0, m1, pct)
        start_step = end_step
    raise AssertionError("unreachable")


class GaussianRampUp:
    """GaussianRampUpScheduler: 0 before start_steps, exp(-5 (1 - x)^2) with x the fraction of the way to end_steps,
    1 from end_steps on."""

    def __init__(self, max_steps, start_steps=None, end_steps=None):
        self.max_steps = max_steps
        self.start_steps = 0 if start_steps is None else start_steps
        self.end_steps = max_steps if end_steps is None else end_steps
        self.curr_steps = 0

    def __call__(self):
        if self.curr_steps < self.start_steps:
            return 0
        if self.curr_steps < self.end_steps:
            x = (self.curr_steps - self.start_steps) / (self.end_steps - self.start_steps)
            return math.exp(-5 * (1 - x) ** 2)
        return 1

    def step(self):
        self.curr_steps += 1

    def resume(self, global_step):
        self.curr_steps = global_step


class NoneScheduler:
    """The weight of a loss without a ramp-up: always 1."""

    def __call__(self):
        return 1

    def step(self):
        pass

    def resume(self, global_step):
        pass
