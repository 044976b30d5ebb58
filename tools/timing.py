"""What the time_*.py tools share: the repository on sys.path, a sample between two device events, its statistics, and the
loop that alternates the variants.  Imported first by each of them (`from timing import ...`)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "iterative-closest-point-avmi_amd"))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def sample(fn, block):
    """``block`` runs of ``fn`` back to back between two device events -> ms per run"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(block):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / block


def stats(v):
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4),
            "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4), "samples": len(v)}


def alternate(variants, samples, warm):
    """``variants``: {name: (fn, runs per sample)}.  Each is warmed by one sample of ``warm`` runs, then ``samples`` rounds take
    one sample of every variant in the dict's order -> {name: [ms per run]}"""
    for fn, _ in variants.values():
        sample(fn, warm)
    times = {name: [] for name in variants}
    for _ in range(samples):
        for name, (fn, block) in variants.items():
            times[name].append(sample(fn, block))
    return times
