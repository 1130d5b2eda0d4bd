"""The expectation semiring (nfst_expectation) against the forward-backward step of the same batch,
on the BASELINE batch (synth.bench_batch(256)) and on 64 SNIPS-shaped lattices.  Writes profiles/expectation.json:

  forward_backward      ops.forward_backward (log alpha, log beta, log Z, arc posteriors): the reference step
  log_z_fwd_bwd         ops.log_z(theta).sum().backward(): the first-order training step
  expectation_launch    ops.expectation_terms with score_coef = 1 and c_a: the three kernels of nfst_expectation alone
  entropy_fwd           ops.entropy without autograd
  entropy_fwd_bwd       ops.entropy(theta).sum().backward()
  log_z_hvp             grad(log_z) with create_graph=True, then grad of <that, u>: a Hessian-vector product of log Z

Cold, as bench.py measures: ROTATE copies of the batch are resident and take turns, so that no launch finds the data of
the previous one in the caches.  Every call is timed with CUDA events around it (GPU time, incl. gaps between its
launches) and host wall time to the end of a synchronise after it; medians of ITERS calls.  The kernels alone:
rocprofv3 --kernel-trace --stats of the same command (profiles/expectation_kernel_stats.csv; see profiles/README.md)."""
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

ITERS = int(os.environ.get("ITERS", "20"))
ROTATE = int(os.environ.get("ROTATE", "4"))
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
    u = torch.randn(theta.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows),
         "max_tiles": int(lat0.max_tiles), "max_depth": int(lat0.depth.max()), "rotate": ROTATE}

    def fb(lat):
        return lambda: ops.forward_backward(lat, theta)

    def lz(lat):
        def f():
            t = theta.clone().requires_grad_()
            ops.log_z(lat, t).sum().backward()
        return f

    def ex(lat):
        return lambda: ops.expectation_terms(lat, theta, score_coef=1.0, want_cov=True, want_label_cov=True)

    def ent(lat):
        return lambda: ops.entropy(lat, theta)

    def ent_bwd(lat):
        def f():
            t = theta.clone().requires_grad_()
            ops.entropy(lat, t).sum().backward()
        return f

    def hvp(lat):
        def f():
            t = theta.clone().requires_grad_()
            (g,) = torch.autograd.grad(ops.log_z(lat, t).sum(), t, create_graph=True)
            torch.autograd.grad((g * u).sum(), t)
        return f

    for key, mk in (("forward_backward", fb), ("log_z_fwd_bwd", lz), ("expectation_launch", ex), ("entropy_fwd", ent),
                    ("entropy_fwd_bwd", ent_bwd), ("log_z_hvp", hvp)):
        r[key] = timed([mk(lat) for lat in copies])
    r["ratio_entropy_fwd_bwd_over_forward_backward"] = round(r["entropy_fwd_bwd"]["event_ms"] / r["forward_backward"]["event_ms"], 3)
    r["ratio_hvp_over_log_z_fwd_bwd"] = round(r["log_z_hvp"]["event_ms"] / r["log_z_fwd_bwd"]["event_ms"], 3)
    print(name, json.dumps(r), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8))
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "expectation.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
