"""Reference-generated fixture of the learning-rate schedules (gfv/schedule.py, csrc/sched.hip gfv_lr_schedule): the rates the
REFERENCE's own classes (utils/scheduler.py: StepexpLRScheduler, ExpLR, GradualStepExplrScheduler) put into a torch optimiser when
driven as its drivers drive them - `optimizer.step(); scheduler.step()` - epoch by epoch from 0 to past total_epoch.

Recorded per case: the kind, the arguments (plain numbers) and the list of rates as hex strings of the doubles; nothing else.
Cases: the drivers' own configuration (pre_train_Adam.py:79-90: milestones at 0.1 and 0.5 of n_epochs, steplr_gamma 1, explr_gamma
1e-1, min_lr 1e-6) at a small n_epochs; steplr_gamma != 1; min_lr above the base rate (the max(..., 0) clamp); a base rate that
is not startlr; ExpLR; GradualStepExplrScheduler with 0, 1 and 8 milestones (one of them at epoch 0, one at total_epoch); and
the warm-up of its plateau branch with multiplier 1 and 2, handing over to torch's ReduceLROnPlateau on a metric series.
Run: python tests/golden/make_golden_sched.py"""
import contextlib
import importlib
import io
import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "refstubs"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

N_EPOCHS = 20     # the drivers' n_epochs, small
# name -> (kind, base_lr, arguments, epochs recorded)
CASES = {
    "stepexp_driver": ("stepexp", 1e-3, dict(startlr=1e-3, steplr_milestone=int(N_EPOCHS * 0.1), steplr_gamma=1,
                                             explr_milestone=int(N_EPOCHS * 0.5), explr_gamma=1e-1, total_epoch=N_EPOCHS,
                                             min_lr=1e-6), N_EPOCHS + 3),
    "stepexp_gamma": ("stepexp", 1e-3, dict(startlr=1e-3, steplr_milestone=3, steplr_gamma=0.3, explr_milestone=7,
                                            explr_gamma=1e-2, total_epoch=13, min_lr=1e-6), 16),
    "stepexp_min_above": ("stepexp", 1e-3, dict(startlr=1e-3, steplr_milestone=2, steplr_gamma=0.5, explr_milestone=5,
                                                explr_gamma=1e-1, total_epoch=9, min_lr=1e-2), 12),
    "stepexp_other_base": ("stepexp", 7e-4, dict(startlr=1e-3, steplr_milestone=0, steplr_gamma=0.9, explr_milestone=4,
                                                 explr_gamma=0.2, total_epoch=11, min_lr=1e-6), 14),
    "exp_default": ("exp", 1e-3, dict(decay_steps=7, gamma=0.4, min_lr=1e-7), 18),
    "exp_min_above": ("exp", 1e-4, dict(decay_steps=3.5, gamma=0.4, min_lr=1e-3), 6),
    "gradual_0": ("gradual", 1e-3, dict(multiplier=1.0, milestone=[], gamma=0.1, expgamma=1e-2, total_epoch=6, decay_steps=9,
                                        min_lr=1e-6), 10),
    "gradual_1": ("gradual", 1e-3, dict(multiplier=1.0, milestone=[4], gamma=0.1, expgamma=1e-2, total_epoch=8, decay_steps=12,
                                        min_lr=1e-6), 12),
    "gradual_8": ("gradual", 1e-3, dict(multiplier=1.0, milestone=[0, 2, 3, 5, 8, 9, 11, 12], gamma=0.7, expgamma=1e-2,
                                        total_epoch=12, decay_steps=5, min_lr=1e-6), 16),
    "gradual_min_above": ("gradual", 1e-4, dict(multiplier=1.0, milestone=[1], gamma=0.5, expgamma=0.3, total_epoch=3,
                                                decay_steps=2, min_lr=1e-3), 7),
}
# the plateau branch: the metric series is given as fp32 values (what a device loss word can hold)
METRICS = [1.0, 0.9, 0.89999, 0.95, 0.96, 0.97, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 0.49999, 0.3]
WARMUP_CASES = {
    "warmup_mult1": (1e-3, dict(multiplier=1.0, warmup_epochs=4), dict(factor=0.5, patience=1, threshold=1e-3, cooldown=1,
                                                                       min_lr=1e-5, eps=1e-8)),
    "warmup_mult2": (1e-3, dict(multiplier=2.0, warmup_epochs=3), dict(factor=0.1, patience=0, threshold=1e-4, cooldown=0,
                                                                       min_lr=0.0, eps=1e-8)),
}


def _optimizer(lr):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr)


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def main():
    import ref_import
    ref_import.install()
    S = importlib.import_module("utils.scheduler")
    out = {"cases": {}, "warmup": {}}
    for name, (kind, base_lr, args, n) in CASES.items():
        opt = _optimizer(base_lr)
        if kind == "stepexp":
            sch = S.StepexpLRScheduler(optimizer=opt, **args)
        elif kind == "exp":
            sch = S.ExpLR(opt, **args)
        else:
            sch = S.GradualStepExplrScheduler(opt, after_scheduler=None, **args)
        rates = []
        for _ in range(n):
            rates.append(float(opt.param_groups[0]["lr"]))
            opt.step()
            sch.step()
        out["cases"][name] = {"kind": kind, "base_lr": base_lr, "args": args, "rates": [r.hex() for r in rates]}
        print(name, ["%.4g" % r for r in rates])
    metrics = [_f32(m) for m in METRICS]
    for name, (base_lr, warm, plat) in WARMUP_CASES.items():
        opt = _optimizer(base_lr)
        after = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", threshold_mode="rel", **plat)
        with contextlib.redirect_stdout(io.StringIO()):
            sch = S.GradualStepExplrScheduler(opt, multiplier=warm["multiplier"], milestone=[], gamma=1.0, after_scheduler=after,
                                              expgamma=1.0, total_epoch=warm["warmup_epochs"], decay_steps=1, min_lr=plat["min_lr"])
            rates = [float(opt.param_groups[0]["lr"])]
            for m in metrics:
                opt.step()
                sch.step(metrics=m)
                rates.append(float(opt.param_groups[0]["lr"]))
        assert all(math.isfinite(r) for r in rates)
        out["warmup"][name] = {"base_lr": base_lr, "warmup": warm, "plateau": plat, "metrics": [m.hex() for m in metrics],
                               "rates": [r.hex() for r in rates]}
        print(name, ["%.4g" % r for r in rates])
    path = os.path.join(HERE, "lr_schedules.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote lr_schedules.json:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
