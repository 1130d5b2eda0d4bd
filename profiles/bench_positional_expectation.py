"""Expectations under position-dependent scores (nfst_positional_expectation) next to the
posterior launch it extends.  Writes profiles/positional_expectation.json.  The protocol and the two batches are those of
profiles/bench_positional.py: the BASELINE batch (synth.bench_batch(256)) and 64 SNIPS-shaped lattices; T is the batch's
depth and every lattice has its own random pos_scores [B, T, V] and cost [B, T, V].

  terms_all        ops.positional_expectation_terms with pos_values and all four optional outputs
  entropy          ops.positional_entropy forward (score_coef = 1, log Z and E[V] only: the backward-in-time pass alone)
  entropy_step     ... forward and backward into theta and pos_scores
  risk_step        ops.positional_expectation(pos_values=cost).sum().backward() into theta and pos_scores
  posteriors       ops.positional_forward_backward with both posteriors   (the yardstick of terms_all)
  log_z            ops.positional_forward_backward without posteriors      (the yardstick of entropy)

Every call is timed with CUDA events around it and host wall time to the end of a synchronise after it; medians of ITERS
calls.  Warm: one resident copy of the inputs, call after call.  Cold: ROTATE copies (batch, pos_scores and cost) take
turns, so that no launch finds the data of the previous one in the caches."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import _lib, ops, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "10"))
ROTATE = int(os.environ.get("ROTATE", "3"))
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


def measure(name, lats, theta_np):
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    B, V, T = lat0.n_lattices, lat0.vocab, int(lat0.depth.max())
    theta = torch.from_numpy(theta_np).to(dev)
    gen = lambda k: torch.Generator(dev).manual_seed(k)
    poss = [torch.randn(B, T, V, device=dev, generator=gen(k)) for k in range(ROTATE)]
    costs = [(torch.rand(B, T, V, device=dev, generator=gen(100 + k)) < 0.9).float() for k in range(ROTATE)]
    bs = C.byref(lat0.c_struct())
    r = {"lattices": B, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "T": T, "rotate": ROTATE,
         "ws_bytes": int(_lib.lib.nfst_positional_expectation_ws_bytes(bs, T)),
         "ws_bytes_posteriors": int(_lib.lib.nfst_positional_ws_bytes(bs, T, _lib.POS_WS_POSTERIOR)),
         "stored_row_bytes": 20 * (T + 1) * int(lat0.total_rows),
         "staged": bool(ops.positional_expectation_plan(lat0)[1]), "staged_posteriors": bool(ops.positional_plan(lat0)[1]),
         "lds_bytes": int(ops.positional_expectation_plan(lat0)[0]), "lds_bytes_posteriors": int(ops.positional_plan(lat0)[0])}

    def auto(fn, lat, pos, cost):
        def f():
            t, p = theta.clone().requires_grad_(), pos.clone().requires_grad_()
            fn(lat, t, p, cost).sum().backward()
        return f

    ops_ = {
        "terms_all": lambda lat, pos, cost: lambda: ops.positional_expectation_terms(
            lat, theta, pos, pos_values=cost, want_pos_posterior=True, want_arc_posterior=True, want_pos_cov=True, want_arc_cov=True),
        "entropy": lambda lat, pos, cost: lambda: ops.positional_entropy(lat, theta, pos),
        "entropy_step": lambda lat, pos, cost: auto(lambda l, t, p, c: ops.positional_entropy(l, t, p), lat, pos, cost),
        "risk_step": lambda lat, pos, cost: auto(lambda l, t, p, c: ops.positional_expectation(l, t, p, pos_values=c), lat, pos, cost),
        "posteriors": lambda lat, pos, cost: lambda: ops.positional_forward_backward(lat, theta, pos, want_arc_posterior=True),
        "log_z": lambda lat, pos, cost: lambda: ops.positional_forward_backward(lat, theta, pos, want_pos_posterior=False),
    }
    for key, make in ops_.items():
        fns = [make(lat, pos, cost) for lat, pos, cost in zip(copies, poss, costs)]
        r[key] = {"warm": timed(fns[:1], ITERS), "cold": timed(fns, ITERS)}
        print(name, key, json.dumps(r[key]), flush=True)
    for key, base in (("terms_all", "posteriors"), ("entropy", "log_z"), ("entropy_step", "posteriors"), ("risk_step", "posteriors")):
        r[f"cold_ratio_{key}_over_{base}"] = round(r[key]["cold"]["event_ms"] / r[base]["cold"]["event_ms"], 2)
    # the masses ride unchanged (a sanity check of the measurement, not a test)
    a = ops.positional_expectation_terms(lat0, theta, poss[0], pos_values=costs[0], want_pos_posterior=True)
    b = ops.positional_forward_backward(lat0, theta, poss[0])
    r["posterior_bits_equal"] = bool(torch.equal(a.pos_posterior, b.pos_posterior) and torch.equal(a.logz64, b.logz64))
    print(name, json.dumps(r), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8))
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "positional_expectation.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
