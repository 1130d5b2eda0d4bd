"""Exact draws under position-dependent scores (nfst_positional_sample / nfst_positional_score_paths, DESIGN.md section
4.10).  Writes profiles/positional_sample.json.  Two batches, as profiles/bench_positional.py: the BASELINE batch
(synth.bench_batch(256)) and 64 SNIPS-shaped lattices; T is the batch's depth, every lattice has its own random
pos_scores [B, T, V]; K = 1, 16 and 256 draws per lattice from the op's own Philox stream.

  log_z        ops.positional_forward_backward(want_pos_posterior=False): the backward pass alone, nothing stored -- the
               yardstick
  sample       the whole op, ops.positional_sample_paths: the backward pass with every beta row stored, then the walks
  beta_rows, walk   the two launches of the op separately: the kernel durations of k_positional and k_positional_walk
               from torch.profiler (null where the profiler gives no kernel records)
  score_paths  ops.positional_score_paths on the drawn paths

Every call is timed with CUDA events around it and host wall time to the end of a synchronise after it; medians of ITERS
calls.  Warm: one resident copy of the inputs, call after call.  Cold: ROTATE copies (batch and pos_scores) take turns,
so that no launch finds the data of the previous one in the caches."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import ops, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "10"))
ROTATE = int(os.environ.get("ROTATE", "3"))
KS = (1, 16, 256)
dev = torch.device(os.environ.get("DEVICE", "cuda"))


def timed(fns, iters):
    fns[0]()
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


def kernel_split(fns, iters):
    """Median duration (ms) of the two kernels of the op over `iters` cold calls, from the profiler's kernel records."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fns[0]()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for k in range(iters):
                fns[k % len(fns)]()
                torch.cuda.synchronize()
        rows, walk = [], []
        for evt in prof.events():
            name = evt.name
            us = getattr(evt, "device_time", None) or getattr(evt, "cuda_time", 0.0)
            if "k_positional_walk" in name:
                walk.append(us)
            elif "k_positional" in name:
                rows.append(us)
        if len(rows) < iters or len(walk) < iters:
            return {"beta_rows_ms": None, "walk_ms": None, "note": f"{len(rows)} and {len(walk)} kernel records for {iters} calls"}
        return {"beta_rows_ms": round(statistics.median(rows) / 1e3, 4), "walk_ms": round(statistics.median(walk) / 1e3, 4)}
    except Exception as exc:  # (a build of torch without a working device profiler: the whole-op timings stand alone)
        return {"beta_rows_ms": None, "walk_ms": None, "note": f"{type(exc).__name__}: {exc}"}


def measure(name, lats, theta_np):
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    B, V, T = lat0.n_lattices, lat0.vocab, int(lat0.depth.max())
    theta = torch.from_numpy(theta_np).to(dev)
    poss = [torch.randn(B, T, V, device=dev, generator=torch.Generator(dev).manual_seed(k)) for k in range(ROTATE)]
    r = {"lattices": B, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "T": T, "rotate": ROTATE,
         "stored_row_bytes": 12 * (T + 1) * int(lat0.total_rows)}
    fns = [lambda lat=lat, pos=pos: ops.positional_forward_backward(lat, theta, pos, want_pos_posterior=False) for lat, pos in zip(copies, poss)]
    r["log_z"] = {"warm": timed(fns[:1], ITERS), "cold": timed(fns, ITERS)}
    print(name, "log_z", json.dumps(r["log_z"]), flush=True)
    for K in KS:
        fns = [lambda lat=lat, pos=pos: ops.positional_sample_paths(lat, theta, K, pos, seed=K) for lat, pos in zip(copies, poss)]
        e = {"sample": {"warm": timed(fns[:1], ITERS), "cold": timed(fns, ITERS)}, "kernels_cold": kernel_split(fns, ITERS)}
        draws = [f().paths for f in fns]
        sfns = [lambda lat=lat, pos=pos, d=d: ops.positional_score_paths(lat, theta, d, pos) for lat, pos, d in zip(copies, poss, draws)]
        e["score_paths"] = {"warm": timed(sfns[:1], ITERS), "cold": timed(sfns, ITERS)}
        e["cold_ratio_sample_over_log_z"] = round(e["sample"]["cold"]["event_ms"] / r["log_z"]["cold"]["event_ms"], 2)
        ks = e["kernels_cold"]
        if ks["walk_ms"] is not None:
            e["walk_cheaper_than_beta_rows"] = ks["walk_ms"] < ks["beta_rows_ms"]
        # a sanity check of the measurement, not a test: log p - log q = log Z for every draw
        s = ops.positional_sample_paths(copies[0], theta, K, poss[0], seed=K)
        p = ops.positional_score_paths(copies[0], theta, s.paths, poss[0])[0]
        e["max_abs_iwae_residual"] = float((p - s.logq - s.logz[:, None]).abs().max())
        r[f"K{K}"] = e
        print(name, f"K{K}", json.dumps(e), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8))
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "positional_sample.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
