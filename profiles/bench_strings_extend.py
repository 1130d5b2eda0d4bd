"""Prefix states (nfst_string_prefix_open / _extend / _state_next, decoders.prefix_search(incremental=True); DESIGN.md
section 4.25) next to the routes they replace, in one run.  Writes profiles/strings_extend.json, per workload:

  open                    ops.string_prefix_open: the level pass, the one-column H sweep, the two indexes, az, the read-back
  step_m{M}_t{t}          one PrefixContext.extend + PrefixContext.next on M = 1 / 8 / 64 live prefixes that grow from t - 1
                          to t symbols (the M heaviest prefixes of every length, found by a beam on the states themselves)
  next_m{M}_t{t}          ops.string_next_log_probs on the same M prefixes of t symbols (N = t): what the step replaces
  ratio_m{M}_t{t}         next over step, event times (above 1: the step is faster)
  search_k{k}             decoders.prefix_search at k = 1 / 8 / 64: the first phase alone (reserve = 0, refine_steps = 0) and
                          the whole search, each with incremental=False (the baseline, same run) and True; medians of
                          SEARCH_ITERS calls, and whether the two results are the same bits

on the two batches of profiles/bench_strings_prefix.py (the BASELINE batch with keep = every second label, cut at max_len =
24; 64 edit grids with the output mark, whose strings have at most a few symbols: t = 1, 2 there).  Cold, as bench.py
measures: ROTATE copies of the batch are resident and take turns; CUDA events around every call and host wall time to the
end of a synchronise after it; medians of ITERS calls."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import decoders, ops  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402
from profiles.bench_strings import ITERS, ROTATE, timed, workloads  # noqa: E402

OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "strings_extend.json"))
ONLY = os.environ.get("WORKLOAD", "")
SEARCH_ITERS = int(os.environ.get("SEARCH_ITERS", "3"))
KS = tuple(int(k) for k in os.environ.get("KS", "1,8,64").split(","))


def beam(ctx, M, t):
    """The M heaviest prefixes of t symbols by a beam of M on the states: (the state of t - 1 symbols, the picks (parent,
    symbol) [B, M] that make the prefixes, the prefixes [B, M, t] and their lengths [B, M] (0 for a dead slot))"""
    B, V, dev = ctx.lat.n_lattices, ctx.lat.vocab, ctx.lat.device
    state, rows = ctx.root(M), torch.zeros((B, M, t), dtype=torch.int32, device=dev)
    for i in range(t):
        flat = ctx.next(state).next.reshape(B, M * V)
        order = torch.sort(-flat, dim=1, stable=True).indices[:, :M]
        alive = flat.gather(1, order) > float("-inf")
        parent = torch.where(alive, order // V, torch.full_like(order, -1)).to(torch.int32)
        symbol = (order % V).to(torch.int32)
        rows = rows.gather(1, parent.clamp(min=0).to(torch.int64)[:, :, None].expand(B, M, t)).clone()
        rows[:, :, i] = symbol
        if i < t - 1:
            state = ctx.extend(state, parent, symbol)
    lens = torch.where(parent >= 0, torch.full_like(parent, t), torch.zeros_like(parent))
    return state, parent, symbol, rows, lens


def measure(name):
    make, theta_np, tape = workloads()[name]
    dev = torch.device("cuda")
    copies = [LatticeBatch.from_synth(make(), device=dev) for _ in range(ROTATE)]
    theta = torch.from_numpy(theta_np).to(dev)
    lat0 = copies[0]
    base = name.startswith("baseline")
    max_len = 24 if base else None
    planes = 2 if "marker" in tape else 1
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "vocab": int(lat0.vocab),
         "tape": sorted(tape)[0], "rotate": ROTATE, "search_max_len": max_len, "state_bytes_m64": 8 * planes * 64 * int(lat0.total_rows)}
    r["open"] = timed([lambda lat=lat: ops.string_prefix_open(lat, theta, **tape) for lat in copies])
    print(name, "open", json.dumps(r["open"]), flush=True)
    ctxs = [ops.string_prefix_open(lat, theta, **tape) for lat in copies]
    for M in (1, 8, 64):
        for t in ((1, 8, 24) if base else (1, 2)):
            made = [beam(ctx, M, t) for ctx in ctxs]
            live = round(float((made[0][4] > 0).double().mean()), 3)

            def step(i):
                ctx, (state, parent, symbol, _, _) = ctxs[i], made[i]
                return ctx.next(ctx.extend(state, parent, symbol))

            def full(i):
                _, _, _, rows, lens = made[i]
                return ops.string_next_log_probs(copies[i], theta, rows, lens, **tape)

            a, b = step(0), full(0)
            on = (made[0][4] > 0)
            same = bool(torch.equal(a.next[on], b.next[on]) and torch.equal(a.log_prefix[on], b.log_prefix[on]))
            s = timed([lambda i=i: step(i) for i in range(ROTATE)])
            f = timed([lambda i=i: full(i) for i in range(ROTATE)])
            r[f"step_m{M}_t{t}"], r[f"next_m{M}_t{t}"] = {**s, "live_share": live, "same_bits": same}, f
            r[f"ratio_m{M}_t{t}"] = round(f["event_ms"] / s["event_ms"], 2)
            print(name, M, t, json.dumps(r[f"step_m{M}_t{t}"]), json.dumps(f), r[f"ratio_m{M}_t{t}"], flush=True)
            del made
    del ctxs
    for k in KS:
        out = {}
        for tag, kw in (("first_phase", dict(reserve=0, refine_steps=0)), ("whole", dict())):
            res = {}
            for inc in (False, True):
                t = timed([lambda lat=lat: decoders.prefix_search(lat, theta, k, max_len, incremental=inc, **kw, **tape) for lat in copies],
                          iters=SEARCH_ITERS)
                res[inc] = decoders.prefix_search(lat0, theta, k, max_len, incremental=inc, **kw, **tape)
                out[f"{tag}_{'incremental' if inc else 'full'}"] = t
            out[f"{tag}_same_bits"] = all(bool(torch.equal(x, y)) for x, y in zip(res[False], res[True]))
            out[f"{tag}_ratio"] = round(out[f"{tag}_full"]["event_ms"] / out[f"{tag}_incremental"]["event_ms"], 2)
        r[f"search_k{k}"] = out
        print(name, k, json.dumps(out), flush=True)
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
