"""Alignments to given strings (nfst_string_viterbi and nfst_string_sample) next to what a user
had before them.  Writes profiles/strings_align.json, per workload:

  string_viterbi_m{1,20,64}          ops.string_viterbi on the first M strings of decoders.decode_strings(k = 64): the level
                                     pass, the max sweep (in slices under 1 GiB of workspace), the walks, the status read-back
  string_sample_m{1,20}_k{1,16,64}   ops.string_sample_paths (Philox draws) on the same strings: the level pass, the sum sweep,
                                     K walks per candidate, the status read-back.  "sweep_ms" is ops.string_log_prob of the
                                     same run (the same two launches and a read-back) and "walk_ms" the difference of the
                                     two event times: the walk kernel and the allocation of its outputs
  product_viterbi_m{..}              alternative (a): per candidate WideDFA.marked_sequence / projected_sequence stacked over
  product_sample_m{..}_k{..}         the lattices -> ops.intersect -> ops.viterbi / ops.sample_paths (float32); "failed":
                                     the candidates whose product raised (beyond NFST_MAX_ROWS, or a string that a
                                     lattice does not spell)

on the BASELINE batch (synth.bench_batch(256)) with keep = every second label, and on 64 edit grids with the output mark:
the two batches and the protocol of profiles/bench_strings.py (cold: ROTATE resident copies take turns; CUDA events around
every call and host wall time to the end of a synchronise after it; medians of ITERS calls, of 3 for the alternatives)."""
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

OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "strings_align.json"))
ONLY = os.environ.get("WORKLOAD", "")


def product_loop(lat, theta, strings, lengths, tape, vocab, k):
    """Alternative (a): the best alignment (k == 0) or k draws of every candidate through the product route; returns the
    number of candidates whose product raised."""
    rows, n = strings.cpu().numpy(), lengths.cpu().numpy()
    failed = 0
    for m in range(rows.shape[1]):
        ys = [rows[b, m, :n[b, m]].tolist() for b in range(rows.shape[0])]
        try:
            if "marker" in tape:
                dfa = WideDFA.stack([WideDFA.marked_sequence(vocab, tape["marker"], y) for y in ys])
            else:
                dfa = WideDFA.stack([WideDFA.projected_sequence(vocab, tape["keep"], y) for y in ys])
            prod = ops.intersect(lat, dfa).lattice
            if k:
                ops.sample_paths(prod, theta, k, seed=1)
            else:
                ops.viterbi(prod, theta)
        except (_lib.NfstError, ValueError, RuntimeError):
            failed += 1
    return failed


def measure(name):
    make, theta_np, tape = workloads()[name]
    lats = make()
    dev = torch.device("cuda")
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0, vocab = copies[0], len(theta_np)
    theta = torch.from_numpy(theta_np).to(dev)
    dec = decoders.decode_strings(lat0, theta, 64, **tape)
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "max_depth": int(lat0.depth.max()),
         "tape": sorted(tape)[0], "rotate": ROTATE, "string_len_max": int(dec.lengths.max())}
    N = max(1, int(dec.lengths.max()))

    def alternative(tag, ys, n, k, calls):
        fails = []
        alt = timed([lambda: fails.append(product_loop(lat0, theta, ys, n, tape, vocab, k))], iters=3)
        r[tag] = {**alt, "failed": int(fails[-1]), "calls": calls}
        print(name, tag, json.dumps(r[tag]), flush=True)

    for M in (1, 20, 64):
        ys, n = dec.strings[:, :M, :N].contiguous(), dec.lengths[:, :M].contiguous()
        r[f"string_viterbi_m{M}"] = timed([lambda lat=lat: ops.string_viterbi(lat, theta, ys, n, **tape) for lat in copies])
        sweep = timed([lambda lat=lat: ops.string_log_prob(lat, theta, ys, n, **tape) for lat in copies])
        r[f"string_log_prob_m{M}"] = sweep
        print(name, M, "viterbi", json.dumps(r[f"string_viterbi_m{M}"]), "string_log_prob", json.dumps(sweep), flush=True)
        alternative(f"product_viterbi_m{M}", ys, n, 0, M)
        if M == 64:
            continue
        for K in (1, 16, 64):
            t = timed([lambda lat=lat: ops.string_sample_paths(lat, theta, ys, n, K, seed=1, **tape) for lat in copies])
            r[f"string_sample_m{M}_k{K}"] = {**t, "sweep_ms": sweep["event_ms"], "walk_ms": round(t["event_ms"] - sweep["event_ms"], 4)}
            print(name, M, K, "sample", json.dumps(r[f"string_sample_m{M}_k{K}"]), flush=True)
            alternative(f"product_sample_m{M}_k{K}", ys, n, K, M)
    # the two routes agree where the product fits: the best alignment of the first candidate
    v = ops.string_viterbi(lat0, theta, dec.strings[:, :1, :N].contiguous(), dec.lengths[:, :1].contiguous(), **tape)
    d = ops.string_sample_paths(lat0, theta, dec.strings[:, :1, :N].contiguous(), dec.lengths[:, :1].contiguous(), 16, seed=1, **tape)
    assert bool(torch.isfinite(v.score).all()) and float(((d.score - d.logq) - d.log_num[:, :, None]).abs().max()) <= 1e-9
    assert bool((v.score <= d.log_num + 1e-9).all())
    print(name, json.dumps(r), flush=True)
    return r


def main():
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
