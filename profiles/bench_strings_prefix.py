"""Prefix probabilities and the prefix search (nfst_string_prefix, nfst_string_next, decoders.prefix_search; DESIGN.md
section 4.23) next to ops.string_log_prob and decoders.decode_strings.  Writes profiles/strings_prefix.json, per workload:

  string_log_prob_m{M}    ops.string_log_prob on M = 1 / 20 / 64 candidates (the first M strings of
                          decoders.decode_strings(k = 64), as profiles/bench_strings.py takes them): the level pass, the G
                          sweep, the status read-back
  prefix_m{M}             ops.string_prefix_log_prob on the same rows taken as prefixes: the level pass, the H sweep, the
                          read-back
  next_m{M}               ops.string_next_log_probs on them: the level pass, the H sweep of the empty prefix, the two
                          indexes, the F sweep, the reduction by label, the read-back
  ratio_prefix_m{M}, ratio_next_m{M}   over string_log_prob_m{M}, event times of this run
  decode_strings_k64      decoders.decode_strings(k = 64)
                          (search_k{k} also holds the time and the certified share of the first phase alone, reserve = 0)
  search_k{k}             decoders.prefix_search at k = 1 / 8 / 64 with its defaults (reserve 64, at most 32 steps of the
                          second phase; medians of SEARCH_ITERS calls): time, the steps taken by both phases (calls of
                          string_next_log_probs), the share of lattices certified ``exact``, and against
                          decode_strings(k = 64), both first strings scored again by one ops.string_log_prob call: the
                          lattices where the search's first string has the strictly higher exact log p ("search_better"),
                          the reverse count ("decode_better") and the lattices where both are the same string

on the two batches of profiles/strings.json: the BASELINE batch (synth.bench_batch(256)) with keep = every second label,
and 64 edit grids with the output mark.  The grids are searched to the end (max_len = the longest path); on the BASELINE
batch, whose 64 best paths spell strings of at most 17 symbols while its longest path has 140 marks, the search is cut at
max_len = 24 (what is still open there goes into ``bound``).  MAX_LEN overrides both.

Cold, as bench.py measures: ROTATE copies of the batch are resident and take turns.  Every call is timed with CUDA events
around it and host wall time to the end of a synchronise after it; medians of ITERS calls."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import decoders, ops  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402
from profiles.bench_strings import ITERS, ROTATE, timed, workloads  # noqa: E402

OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "strings_prefix.json"))
ONLY = os.environ.get("WORKLOAD", "")
SEARCH_ITERS = int(os.environ.get("SEARCH_ITERS", "3"))
MAX_LEN = int(os.environ["MAX_LEN"]) if os.environ.get("MAX_LEN") else None
KS = tuple(int(k) for k in os.environ.get("KS", "1,8,64").split(","))


def counted_search(lat, theta, k, max_len, tape):
    """prefix_search and the number of string_next_log_probs calls it made"""
    calls = [0]
    inner = ops.string_next_log_probs

    def counting(*a, **kw):
        calls[0] += 1
        return inner(*a, **kw)

    ops.string_next_log_probs = counting
    try:
        r = decoders.prefix_search(lat, theta, k, max_len, **tape)
    finally:
        ops.string_next_log_probs = inner
    return r, calls[0]


def first_strings_compared(lat, theta, r, dec, tape):
    """Both first strings as two candidates of one string_log_prob call: (search better, decode better, same string)"""
    L = max(r.strings.shape[2], dec.strings.shape[2])
    pad = lambda x: torch.nn.functional.pad(x[:, :1], (0, L - x.shape[2]))
    ys = torch.cat([pad(r.strings), pad(dec.strings)], dim=1)
    n = torch.cat([r.lengths[:, :1], dec.lengths[:, :1]], dim=1)
    lp = ops.string_log_prob(lat, theta, ys, n, **tape).log_prob
    cols = torch.arange(L, device=ys.device)[None, :]
    same = (n[:, 0] == n[:, 1]) & ((ys[:, 0] == ys[:, 1]) | (cols >= n[:, :1])).all(dim=1)
    return int(((lp[:, 0] > lp[:, 1]) & ~same).sum()), int(((lp[:, 1] > lp[:, 0]) & ~same).sum()), int(same.sum())


def measure(name):
    make, theta_np, tape = workloads()[name]
    dev = torch.device("cuda")
    copies = [LatticeBatch.from_synth(make(), device=dev) for _ in range(ROTATE)]
    theta = torch.from_numpy(theta_np).to(dev)
    lat0 = copies[0]
    dec = decoders.decode_strings(lat0, theta, 64, **tape)
    max_len = MAX_LEN if MAX_LEN is not None else (24 if name.startswith("baseline") else None)
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "vocab": int(lat0.vocab),
         "tape": sorted(tape)[0], "rotate": ROTATE, "string_len_max": int(dec.lengths.max()), "search_max_len": max_len}
    N = max(1, int(dec.lengths.max()))
    for M in (1, 20, 64):
        ys, n = dec.strings[:, :M, :N].contiguous(), dec.lengths[:, :M].contiguous()
        slp = timed([lambda lat=lat: ops.string_log_prob(lat, theta, ys, n, **tape) for lat in copies])
        pre = timed([lambda lat=lat: ops.string_prefix_log_prob(lat, theta, ys, n, **tape) for lat in copies])
        nxt = timed([lambda lat=lat: ops.string_next_log_probs(lat, theta, ys, n, **tape) for lat in copies])
        r[f"string_log_prob_m{M}"], r[f"prefix_m{M}"], r[f"next_m{M}"] = slp, pre, nxt
        r[f"ratio_prefix_m{M}"] = round(pre["event_ms"] / slp["event_ms"], 2)
        r[f"ratio_next_m{M}"] = round(nxt["event_ms"] / slp["event_ms"], 2)
        print(name, M, json.dumps(slp), json.dumps(pre), json.dumps(nxt), flush=True)
    r["decode_strings_k64"] = timed([lambda lat=lat: decoders.decode_strings(lat, theta, 64, **tape) for lat in copies], iters=SEARCH_ITERS)
    for k in KS:
        t = timed([lambda lat=lat: decoders.prefix_search(lat, theta, k, max_len, **tape) for lat in copies], iters=SEARCH_ITERS)
        res, steps = counted_search(lat0, theta, k, max_len, tape)
        better, worse, same = first_strings_compared(lat0, theta, res, dec, tape)
        plain = timed([lambda lat=lat: decoders.prefix_search(lat, theta, k, max_len, reserve=0, refine_steps=0, **tape) for lat in copies],
                      iters=SEARCH_ITERS)
        first_phase = decoders.prefix_search(lat0, theta, k, max_len, reserve=0, refine_steps=0, **tape)
        r[f"search_k{k}"] = {**t, "first_phase_alone_event_ms": plain["event_ms"],
                             "first_phase_alone_exact_share": round(float(first_phase.exact.double().mean()), 4), "steps": steps, "exact_share": round(float(res.exact.double().mean()), 4), "search_better": better,
                             "decode_better": worse, "same_first_string": same}
        print(name, k, json.dumps(r[f"search_k{k}"]), json.dumps(r["decode_strings_k64"]), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS, "search_iters": SEARCH_ITERS}
    if os.path.exists(OUT) and ONLY:
        with open(OUT) as f:
            out = json.load(f)
    for name in sorted(workloads(), reverse=True):  # (the grids first)
        if not ONLY or ONLY == name:
            out[name] = measure(name)
            with open(OUT, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
