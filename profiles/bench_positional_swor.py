"""Draws without replacement under positional scores and a length budget (nfst_positional_swor)
next to the draws with replacement under the same scores and the plain draws without replacement of the same batch.
Writes profiles/positional_swor.json.  Two batches, as profiles/bench_positional_sample.py: the BASELINE batch
(synth.bench_batch(256), T = its depth, 140) and 64 SNIPS-shaped lattices (T = 748); every lattice has its own random
pos_scores [B, T, V]; k = 1, 16 and 64 from the op's own Philox stream.

  positional_swor_k{K}     the whole op, swor.positional_sample: the backward pass with every beta row stored, the search,
                           the workspace allocation and the status read-back
  kernels_k{K}             the two launches of the op separately: the kernel durations of k_positional (beta_rows_ms) and
                           k_swor (search_ms) from torch.profiler (null where the profiler gives no kernel records)
  positional_sample_k{K}   ops.positional_sample_paths, K draws with replacement under the same scores
  swor_k{K}                swor.sample with its ops.backward call, under theta alone (no position scores, no budget)
  steps_mean / steps_max   steps of the search per lattice (the longest drawn path), at K = 64
  us_per_step_k{K}         search_ms (the whole op's event time where the profiler gives nothing) over steps_max: every
                           lattice has a workgroup of its own, so the launch lasts as long as its deepest search

and

  max_gumbel_error    the largest |G_gpu - G_ref| and |kappa_gpu - kappa_ref| over the decided lattices of every comparison
                      of tests/test_gpu_positional_swor.py: the reference is fed NumPy beta rows of its own, so the figure
                      includes the difference between the two backward passes (tests/positional_swor_ref.DECIDED stays
                      at least 100 times this value)

Cold, as bench.py measures: ROTATE copies of the batch and of pos_scores are resident and take turns, so that no launch
finds the data of the previous one in the caches.  Every call is timed with CUDA events around it (GPU time, incl. gaps
between its launches) and host wall time to the end of a synchronise after it; medians of ITERS calls."""
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

ITERS = int(os.environ.get("ITERS", "10"))
ROTATE = int(os.environ.get("ROTATE", "3"))
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


def kernel_split(fns, iters=ITERS):
    """Median duration (ms) of the two kernels of the op over `iters` cold calls, from the profiler's kernel records."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fns[0]()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for k in range(iters):
                fns[k % len(fns)]()
                torch.cuda.synchronize()
        rows, search = [], []
        for evt in prof.events():
            us = getattr(evt, "device_time", None) or getattr(evt, "cuda_time", 0.0)
            if "k_swor" in evt.name:
                search.append(us)
            elif "k_positional" in evt.name:
                rows.append(us)
        if len(rows) < iters or len(search) < iters:
            return {"beta_rows_ms": None, "search_ms": None, "note": f"{len(rows)} and {len(search)} kernel records for {iters} calls"}
        return {"beta_rows_ms": round(statistics.median(rows) / 1e3, 4), "search_ms": round(statistics.median(search) / 1e3, 4)}
    except Exception as exc:  # (a build of torch without a working device profiler: the whole-op timings stand alone)
        return {"beta_rows_ms": None, "search_ms": None, "note": f"{type(exc).__name__}: {exc}"}


def measure(name, lats, theta_np):
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    B, V, T = lat0.n_lattices, lat0.vocab, int(lat0.depth.max())
    theta = torch.from_numpy(theta_np).to(dev)
    poss = [torch.randn(B, T, V, device=dev, generator=torch.Generator(dev).manual_seed(k)) for k in range(ROTATE)]
    r = {"lattices": B, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "T": T, "rotate": ROTATE,
         "stored_row_bytes": 12 * (T + 1) * int(lat0.total_rows)}
    for k in KS:
        fns = [lambda lat=lat, pos=pos: swor.positional_sample(lat, theta, k, pos, seed=1) for lat, pos in zip(copies, poss)]
        r[f"positional_swor_k{k}"] = timed(fns)
        r[f"kernels_k{k}"] = kernel_split(fns)
        r[f"positional_sample_k{k}"] = timed([lambda lat=lat, pos=pos: ops.positional_sample_paths(lat, theta, k, pos, seed=1)
                                              for lat, pos in zip(copies, poss)])
        r[f"swor_k{k}"] = timed([(lambda lat=lat: swor.sample(lat, theta, k, seed=1)) for lat in copies])
        print(name, k, json.dumps({n: v for n, v in r.items() if n.endswith(f"_k{k}")}), flush=True)
    res = swor.positional_sample(lat0, theta, 64, poss[0], seed=1)
    steps = res.lengths.max(dim=1).values.double()
    r["steps_mean"], r["steps_max"] = round(float(steps.mean()), 2), int(steps.max())
    r["paths_drawn_k64"] = int(res.n_paths.sum())
    for k in KS:
        search = r[f"kernels_k{k}"]["search_ms"]
        r[f"us_per_step_k{k}"] = round(1e3 * (search if search is not None else r[f"positional_swor_k{k}"]["event_ms"]) / max(r["steps_max"], 1), 2)
    print(name, json.dumps(r), flush=True)
    return r


def gumbel_error():
    """The comparisons of tests/test_gpu_positional_swor.py::test_against_the_reference, reduced to their largest difference."""
    from tests import positional_swor_ref as Q
    from tests import swor_ref as R

    worst, decided, lattices = 0.0, 0, 0
    for name in R.cases():
        lat = None
        for T in Q.case_budgets(name):
            for k in R.cases()[name]().ks:
                case, pos, u, refs = Q.references(name, T, k)
                lat = lat or LatticeBatch.from_synth(case.lats, device=dev, **case.opts)
                asc = None if case.asc is None else torch.from_numpy(case.asc).to(dev)
                res = swor.positional_sample(lat, torch.from_numpy(case.theta).to(dev), k, torch.from_numpy(pos).to(dev), arc_scores=asc,
                                             uniforms=torch.from_numpy(u))
                g, kap = res.gumbel.cpu().numpy(), res.kappa.cpu().numpy()
                for b, ref in enumerate(refs):
                    lattices += 1
                    if not Q.decided(ref):
                        continue
                    decided += 1
                    n = ref["n_paths"]
                    if n:
                        worst = max(worst, float(np.max(np.abs(g[b, :n] - ref["gumbel"]))))
                    if np.isfinite(ref["kappa"]):
                        worst = max(worst, abs(float(kap[b]) - ref["kappa"]))
    return {"max_gumbel_error": worst, "decided_lattices": decided, "compared_lattices": lattices, "decided_margin": Q.DECIDED}


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    out.update(gumbel_error())
    print(json.dumps(out), flush=True)
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8))
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "positional_swor.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
