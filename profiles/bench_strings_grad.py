"""The gradient of ops.string_log_prob (nfst_string_logprob_grad) next to its forward and to what
a user had before it.  Writes profiles/strings_grad.json, per workload and M = 1 / 20 / 64 candidates (the first M strings
of decoders.decode_strings(k = 64), as profiles/bench_strings.py takes them):

  forward_m{M}            ops.string_log_prob without a gradient: the level pass, the G sweep, the status read-back
  forward_backward_m{M}   the same call with theta requiring grad, and log_prob.sum().backward() (the dead candidates
                          masked out): the forward again, then the level pass, the G sweep, the in-arc index, the F sweep,
                          the arc pass and the per-label sums of the theta gradient
  ratio_m{M}              forward_backward over forward, event times of this run
  constraint_loop_m{M}    alternative (a): one ops.constraint_log_prob per candidate with .backward() on its sum, the
                          lattices' automata stacked (float32); "failed": the calls that raised, medians of 3
  kernels_m{M}            the launches of the backward alone: average us per launch of k_kbest_levels, k_string_logprob
                          (G), k_string_logprob_index, k_string_logprob_fwd (F) and k_string_logprob_arcs from
                          ``rocprofv3 --kernel-trace --stats`` of ``WORKLOAD=<name> M=<M> python
                          profiles/bench_strings_grad.py trace`` (a run of its own), merged by ``python
                          profiles/bench_strings_grad.py merge <name> <M> <kernel_stats.csv>``

on the two batches of profiles/strings.json: the BASELINE batch (synth.bench_batch(256)) with keep = every second label,
and 64 edit grids with the output mark.

Cold, as bench.py measures: ROTATE copies of the batch are resident and take turns.  Every call is timed with CUDA events
around it and host wall time to the end of a synchronise after it; medians of ITERS calls (of 3 for the alternative)."""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import _lib, decoders, ops  # noqa: E402
from nfst_amd.constraints import WideDFA  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402
from profiles.bench_strings import ITERS, ROTATE, timed, workloads  # noqa: E402

OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "strings_grad.json"))
ONLY = os.environ.get("WORKLOAD", "")
KERNELS = ("k_kbest_levels", "k_string_logprob", "k_string_logprob_index", "k_string_logprob_fwd", "k_string_logprob_arcs")


def setup(name):
    make, theta_np, tape = workloads()[name]
    dev = torch.device("cuda")
    copies = [LatticeBatch.from_synth(make(), device=dev) for _ in range(ROTATE)]
    theta = torch.from_numpy(theta_np).to(dev)
    dec = decoders.decode_strings(copies[0], theta, 64, **tape)
    return copies, theta, tape, dec


def candidates(dec, M):
    N = max(1, int(dec.lengths.max()))
    return dec.strings[:, :M, :N].contiguous(), dec.lengths[:, :M].contiguous()


def train_step(lat, theta, ys, n, tape):
    th = theta.detach().clone().requires_grad_()
    lp = ops.string_log_prob(lat, th, ys, n, **tape).log_prob
    torch.where(torch.isneginf(lp), torch.zeros_like(lp), lp).sum().backward()
    return th.grad


def constraint_step(lat, theta, strings, lengths, tape, vocab):
    """Alternative (a) with its backward pass; returns the number of calls that raised."""
    rows, n = strings.cpu().numpy(), lengths.cpu().numpy()
    th = theta.detach().clone().requires_grad_()
    failed = 0
    for m in range(rows.shape[1]):
        ys = [rows[b, m, :n[b, m]].tolist() for b in range(rows.shape[0])]
        try:
            if "marker" in tape:
                dfa = WideDFA.stack([WideDFA.marked_sequence(vocab, tape["marker"], y) for y in ys])
            else:
                dfa = WideDFA.stack([WideDFA.projected_sequence(vocab, tape["keep"], y) for y in ys])
            ops.constraint_log_prob(lat, th, dfa).sum().backward()
        except (_lib.NfstError, ValueError, RuntimeError):
            failed += 1
    return failed


def measure(name):
    copies, theta, tape, dec = setup(name)
    lat0, vocab = copies[0], theta.numel()
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "tape": sorted(tape)[0], "rotate": ROTATE,
         "string_len_max": int(dec.lengths.max())}
    for M in (1, 20, 64):
        ys, n = candidates(dec, M)
        fwd = timed([lambda lat=lat: ops.string_log_prob(lat, theta, ys, n, **tape) for lat in copies])
        both = timed([lambda lat=lat: train_step(lat, theta, ys, n, tape) for lat in copies])
        fails = []
        alt = timed([lambda: fails.append(constraint_step(lat0, theta, ys, n, tape, vocab))], iters=3)
        r[f"forward_m{M}"], r[f"forward_backward_m{M}"] = fwd, both
        r[f"ratio_m{M}"] = round(both["event_ms"] / fwd["event_ms"], 2)
        r[f"constraint_loop_m{M}"] = {**alt, "failed": int(fails[-1]), "calls": M}
        print(name, M, json.dumps(fwd), json.dumps(both), r[f"ratio_m{M}"], json.dumps(r[f"constraint_loop_m{M}"]), flush=True)
    # the gradient agrees with the product route where that route works (float32 there)
    ys, n = candidates(dec, 1)
    try:
        th = theta.detach().clone().requires_grad_()
        rows, nn = ys.cpu().numpy(), n.cpu().numpy()
        seq = WideDFA.marked_sequence if "marker" in tape else WideDFA.projected_sequence
        dfa = WideDFA.stack([seq(vocab, tape.get("marker", tape.get("keep")), rows[b, 0, :nn[b, 0]].tolist()) for b in range(rows.shape[0])])
        ops.constraint_log_prob(lat0, th, dfa).sum().backward()
        r["max_abs_theta_grad_difference_to_the_product_route_m1"] = float((train_step(lat0, theta, ys, n, tape) - th.grad).abs().max())
    except (_lib.NfstError, ValueError, RuntimeError) as e:
        r["max_abs_theta_grad_difference_to_the_product_route_m1"] = f"the product route raised: {type(e).__name__}"
    print(name, json.dumps(r), flush=True)
    return r


def trace(name, M):
    """The backward's entry point alone, ITERS cold calls behind one warm-up per copy: the command rocprofv3 traces."""
    from nfst_amd import strings

    copies, theta, tape, dec = setup(name)
    ys, n = candidates(dec, M)
    B = copies[0].n_lattices
    g_num, g_z = torch.ones((B, M), dtype=torch.float64, device="cuda"), -torch.ones(B, dtype=torch.float64, device="cuda") * M

    def one(lat):
        c = strings._candidates(lat, ys, n, tape.get("keep"), tape.get("marker"), 1 << 30)
        sc, alive = ops._scores(lat, theta, None)
        return strings._grad_launches(c, sc, g_num, g_z), alive

    timed([lambda lat=lat: one(lat) for lat in copies])


def merge(name, M, stats_csv):
    with open(OUT) as f:
        out = json.load(f)
    k = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            for kn in KERNELS:
                if any(kn + tail in row["Name"] for tail in ("(", "<true>(", "<false>(")):
                    k[kn] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 1),
                             "min_us": round(float(row["MinNs"]) / 1e3, 1), "max_us": round(float(row["MaxNs"]) / 1e3, 1)}
    out[name][f"kernels_m{M}"] = k
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(os.environ["WORKLOAD"], int(os.environ.get("M", "20")))
    if len(sys.argv) > 1 and sys.argv[1] == "merge":
        return merge(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    if os.path.exists(OUT) and ONLY:
        with open(OUT) as f:
            out = json.load(f)
    for name in workloads():
        if not ONLY or ONLY == name:
            out[name] = measure(name)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
