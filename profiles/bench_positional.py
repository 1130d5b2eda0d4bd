"""Position-dependent scores (nfst_positional / nfst_positional_viterbi) next to two baselines.
Writes profiles/positional.json.  Two batches: the BASELINE batch (synth.bench_batch(256)) and 64 SNIPS-shaped lattices;
T is the batch's depth and every lattice has its own random pos_scores [B, T, V].

  log_z            ops.positional_forward_backward without posteriors (the backward-in-time pass alone)
  posteriors       ... with the position and the arc posteriors (both passes, every beta row stored)
  viterbi          ops.positional_viterbi
  autograd_step    ops.positional_log_z(...).sum().backward() into theta and pos_scores
  forward_backward ops.forward_backward on the same batch (no position scores: what the engine could do before)
  torch_log_z      the same log Z composed from torch ops: a T-step loop of gather, add and scatter-logsumexp over the arc
                   list -- what a user can write today; torch_autograd_step: its forward and backward (the posteriors);
                   torch_max: the same loop with amax (the best score, no path)

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
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfst_amd import ops, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "10"))
TORCH_ITERS = int(os.environ.get("TORCH_ITERS", "3"))
ROTATE = int(os.environ.get("ROTATE", "3"))
dev = torch.device(os.environ.get("DEVICE", "cuda"))
NEG = float("-inf")


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


class TorchLoop:
    """log Z_T (or the best score) as a user composes it from torch ops on the arc list."""

    def __init__(self, lat):
        keep = (lat.arc_src != lat.arc_dst).nonzero().squeeze(1)
        b = lat.arc_lattice()[keep]
        ro = torch.from_numpy(lat.row_off.astype(np.int64)).to(dev)
        self.b, self.lab = b, lat.arc_label[keep].long()
        self.src, self.dst = lat.arc_src[keep].long() + ro[b], lat.arc_dst[keep].long() + ro[b]
        self.start, self.sink = ro, ro + torch.from_numpy(lat.sink.astype(np.int64)).to(dev)
        self.rows, self.B = int(lat.total_rows), lat.n_lattices

    def __call__(self, theta, pos, maximum=False):
        T = pos.shape[1]
        alpha = torch.full((self.rows,), NEG, device=dev).index_put((self.start,), torch.zeros(self.B, device=dev))
        ends = []
        for t in range(T):
            term = alpha[self.src] + theta[self.lab] + pos[self.b, t, self.lab]
            m = torch.full((self.rows,), NEG, device=dev).scatter_reduce(0, self.dst, term, "amax")
            if maximum:
                nxt = m
            else:
                ms = torch.where(torch.isfinite(m), m, torch.zeros_like(m)).detach()
                nxt = torch.zeros(self.rows, device=dev).index_add(0, self.dst, torch.exp(term - ms[self.dst])).log() + ms
            ends.append(nxt[self.sink])
            alpha = nxt.index_put((self.sink,), torch.full((self.B,), NEG, device=dev))
        ends = torch.stack(ends)
        return ends.amax(dim=0) if maximum else torch.logsumexp(ends, dim=0)


def measure(name, lats, theta_np):
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    B, V, T = lat0.n_lattices, lat0.vocab, int(lat0.depth.max())
    theta = torch.from_numpy(theta_np).to(dev)
    poss = [torch.randn(B, T, V, device=dev, generator=torch.Generator(dev).manual_seed(k)) for k in range(ROTATE)]
    r = {"lattices": B, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "T": T, "rotate": ROTATE,
         "stored_row_bytes": 12 * (T + 1) * int(lat0.total_rows)}
    loops = [TorchLoop(lat) for lat in copies]

    def auto(fn, lat, pos):
        def f():
            t, p = theta.clone().requires_grad_(), pos.clone().requires_grad_()
            fn(lat, t, p).sum().backward()
        return f

    ops_ = {
        "log_z": lambda lat, pos, lp: lambda: ops.positional_forward_backward(lat, theta, pos, want_pos_posterior=False),
        "posteriors": lambda lat, pos, lp: lambda: ops.positional_forward_backward(lat, theta, pos, want_arc_posterior=True),
        "viterbi": lambda lat, pos, lp: lambda: ops.positional_viterbi(lat, theta, pos),
        "autograd_step": lambda lat, pos, lp: auto(ops.positional_log_z, lat, pos),
        "forward_backward": lambda lat, pos, lp: lambda: ops.forward_backward(lat, theta, want_alpha_beta=False),
        "torch_log_z": lambda lat, pos, lp: lambda: lp(theta, pos),
        "torch_max": lambda lat, pos, lp: lambda: lp(theta, pos, maximum=True),
        "torch_autograd_step": lambda lat, pos, lp: auto(lambda _l, t, p: lp(t, p), lat, pos),
    }
    for key, make in ops_.items():
        n = TORCH_ITERS if key.startswith("torch") else ITERS
        fns = [make(lat, pos, lp) for lat, pos, lp in zip(copies, poss, loops)]
        r[key] = {"warm": timed(fns[:1], n), "cold": timed(fns, n)}
        print(name, key, json.dumps(r[key]), flush=True)
    # the two compositions agree (a sanity check of the baseline, not a test)
    z = ops.positional_forward_backward(lat0, theta, poss[0], want_pos_posterior=False).logz64
    r["max_abs_diff_to_torch_log_z"] = float((z - loops[0](theta, poss[0]).double()).abs().max())
    for key, base in (("log_z", "torch_log_z"), ("posteriors", "torch_autograd_step"), ("autograd_step", "torch_autograd_step"),
                      ("viterbi", "torch_max")):
        r[f"cold_ratio_torch_over_{key}"] = round(r[base]["cold"]["event_ms"] / r[key]["cold"]["event_ms"], 2)
        r[f"cold_ratio_{key}_over_forward_backward"] = round(r[key]["cold"]["event_ms"] / r["forward_backward"]["cold"]["event_ms"], 2)
    print(name, json.dumps(r), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS, "torch_iters": TORCH_ITERS}
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8))
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "positional.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
