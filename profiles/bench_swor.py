"""Draws without replacement (nfst_swor) next to the draws with replacement and the k best paths
of the same batch.  Writes profiles/swor.json:

  backward            ops.backward (log beta and log Z: what every draw below needs first)
  swor_k{K}           swor.sample at K = 1, 16, 64 given the backward result (one launch, the workspace allocation and
                      the status read-back)
  swor_k{K}_with_backward  the same with the ops.backward call in front of it
  sample_paths_k{K}   ops.sample_paths, K draws with replacement, given its backward result; ..._with_backward as above
  k_best_k{K}         ops.k_best
  steps_mean / steps_max   steps of the search per lattice (the longest drawn path), at K = 64
  us_per_step_k{K}    swor_k{K}'s event time over steps_max: every lattice has a workgroup of its own, so the launch lasts
                      as long as its deepest search (over steps_mean: us_per_mean_step_k{K})

on the BASELINE batch (synth.bench_batch(256)) and on 64 SNIPS-shaped lattices, and

  max_gumbel_error    the largest |G_gpu - G_ref| and |kappa_gpu - kappa_ref| over the decided lattices of every case of
                      tests/swor_ref.py, the reference fed the op's own log beta (tests/swor_ref.DECIDED stays at
                      least 100 times this value)

Cold, as bench.py measures: ROTATE copies of the batch are resident and take turns, so that no launch finds the data of
the previous one in the caches.  Every call is timed with CUDA events around it (GPU time, incl. gaps between its
launches) and host wall time to the end of a synchronise after it; medians of ITERS calls."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfst_amd import ops, swor, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "20"))
ROTATE = int(os.environ.get("ROTATE", "4"))
KS = (1, 16, 64)
dev = torch.device("cuda")


def timed(fns, iters=ITERS):
    """fns: one callable per resident copy; call k runs fns[k % len(fns)]."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ev, wall = [], []
    for k in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        fns[k % len(fns)]()
        e.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(s.elapsed_time(e))
    return {"event_ms": round(statistics.median(ev), 4), "wall_ms": round(statistics.median(wall), 4)}


def measure(name, lats, theta_np):
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    theta = torch.from_numpy(theta_np).to(dev)
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows),
         "max_depth": int(lat0.depth.max()), "rotate": ROTATE}
    betas = [ops.backward(lat, theta) for lat in copies]
    betas_me = [ops.backward(lat, theta, want_logbeta=False, want_me=True) for lat in copies]
    r["backward"] = timed([(lambda lat=lat: ops.backward(lat, theta)) for lat in copies])
    for k in KS:
        r[f"swor_k{k}"] = timed([(lambda lat=lat, b=b: swor.sample(lat, theta, k, seed=1, beta=b)) for lat, b in zip(copies, betas)])
        r[f"swor_k{k}_with_backward"] = timed([(lambda lat=lat: swor.sample(lat, theta, k, seed=1)) for lat in copies])
        r[f"sample_paths_k{k}"] = timed([(lambda lat=lat, b=b: ops.sample_paths(lat, theta, k, seed=1, beta=b))
                                         for lat, b in zip(copies, betas_me)])
        r[f"sample_paths_k{k}_with_backward"] = timed([(lambda lat=lat: ops.sample_paths(lat, theta, k, seed=1)) for lat in copies])
        r[f"k_best_k{k}"] = timed([(lambda lat=lat: ops.k_best(lat, theta, k)) for lat in copies])
    steps = swor.sample(lat0, theta, 64, seed=1, beta=betas[0]).lengths.max(dim=1).values.double()
    r["steps_mean"], r["steps_max"] = round(float(steps.mean()), 2), int(steps.max())
    for k in KS:
        r[f"us_per_step_k{k}"] = round(1e3 * r[f"swor_k{k}"]["event_ms"] / r["steps_max"], 2)
        r[f"us_per_mean_step_k{k}"] = round(1e3 * r[f"swor_k{k}"]["event_ms"] / r["steps_mean"], 2)
    print(name, json.dumps(r), flush=True)
    return r


def gumbel_error():
    """The comparison of tests/test_gpu_swor.py, reduced to its largest difference."""
    from tests import swor_ref as R

    worst, decided, lattices = 0.0, 0, 0
    for name, make in R.cases().items():
        case = make()
        lat = LatticeBatch.from_synth(case.lats, device=dev, **case.opts)
        theta = torch.from_numpy(case.theta).to(dev)
        asc = None if case.asc is None else torch.from_numpy(case.asc).to(dev)
        L = int(lat.depth.max()) + 1
        for k in case.ks:
            u = case.uniforms(k, L)
            beta = ops.backward(lat, theta, asc)
            res = swor.sample(lat, theta, k, arc_scores=asc, max_len=L, uniforms=torch.from_numpy(u), beta=beta)
            lb, z = beta.logbeta.cpu().numpy(), beta.logz64.cpu().numpy()
            bs = [(lb[int(lat.row_off[b]):int(lat.row_off[b]) + int(lat.n_rows[b])], float(z[b])) for b in range(lat.n_lattices)]
            g, kap = res.gumbel.cpu().numpy(), res.kappa.cpu().numpy()
            for b, ref in enumerate(case.references(k, betas=bs, uniforms=u, max_len=L)):
                lattices += 1
                if not R.decided(ref):
                    continue
                decided += 1
                n = ref["n_paths"]
                if n:
                    worst = max(worst, float(np.max(np.abs(g[b, :n] - ref["gumbel"]))))
                if np.isfinite(ref["kappa"]):
                    worst = max(worst, abs(float(kap[b]) - ref["kappa"]))
    return {"max_gumbel_error": worst, "decided_lattices": decided, "compared_lattices": lattices, "decided_margin": R.DECIDED}


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    out.update(gumbel_error())
    print(json.dumps(out), flush=True)
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8))
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "swor.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
