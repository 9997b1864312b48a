"""The fp64 yardstick shared by the element-wise parity tests (test_gpu_train_geometry.py, test_gpu_recurrence.py,
test_recurrence_oracle.py): each tensor is held to the fp32 CPU oracle's own error on it,

    max|x_hip - x64| <= min(M * max|x32 - x64| + floor * max|x64|,  CAP * max|x64|)

Running `pytest -s` prints every comparison ("PARITY" lines) and the worst of each case ("PARITY-WORST")."""
import torch

FLOOR = 1e-5
CAP = 1e-3


class Checker:
    """Collects every comparison (for the calibration table) and every violation (reported together at the end)."""

    def __init__(self, case, m, floor=FLOOR):
        self.case, self.m, self.floor, self.rows, self.bad = case, m, floor, [], []

    def __call__(self, name, hip, x32, x64):
        hip, x32, x64 = hip.detach().cpu().double().flatten(), x32.detach().double().flatten(), x64.detach().double().flatten()
        assert hip.shape == x64.shape, (name, hip.shape, x64.shape)
        assert bool(torch.isfinite(hip).all()), name
        scale = float(x64.abs().max())
        e_hip, e32 = float((hip - x64).abs().max()), float((x32 - x64).abs().max())
        bound = min(self.m * e32 + self.floor * scale, CAP * scale)
        need = max(0.0, e_hip - self.floor * scale) / e32 if e32 > 0 else (0.0 if e_hip <= self.floor * scale else float("inf"))
        self.rows.append((name, e_hip / scale if scale else e_hip, e32 / scale if scale else e32, need))
        if not e_hip <= bound:
            self.bad.append("%s: max|hip-64| %.3e > bound %.3e (max|64| %.3e, max|32-64| %.3e)" % (name, e_hip, bound, scale, e32))

    def finish(self):
        for name, rel, rel32, need in self.rows:
            print("PARITY %s %s rel_hip=%.3e rel_32=%.3e need_m=%.3g" % (self.case, name, rel, rel32, need))
        worst = max(self.rows, key=lambda r: r[3])
        print("PARITY-WORST %s %s need_m=%.3g" % (self.case, worst[0], worst[3]))
        assert not self.bad, "%s:\n  " % self.case + "\n  ".join(self.bad)
