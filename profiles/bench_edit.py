"""Edit distance over drawn path sets (nfst_edit_distance) next to the two ways a user had
before it.  Writes profiles/edit.json; per batch and per K = 1, 16, 64 (K paths per lattice drawn by swor.sample):

  gold_k{K}       ops.edit_distance of the set to one gold row per lattice (another draw): [B, K] distances
  pairwise_k{K}   ops.pairwise_edit_distance: [B, K, K]
  mbr_k{K}        decoders.mbr_decode of the drawn set (the pairwise launch, the Horvitz-Thompson weights, the selection)
  ..._torch       (a) the same numbers from a torch composition on the GPU: every pair at once, one loop over the rows of
                  the table with t = min(prev + 1, shifted_prev + neq) and d = cummin(t - j) + j (five launches a row)
  ..._host        (b) the paths copied to the host and a row-vectorised NumPy sweep per lattice on HOST_THREADS threads
                  (the copy is inside the timing)
  cells, gcells_per_s   cells of the dynamic programs (sum of la * lb over the pairs computed: i < j in symmetric mode)
                  and the kernel's cell updates per second of event time

on the BASELINE batch (synth.bench_batch(256), paths of at most 140 marks) and on 64 SNIPS-shaped lattices (at most 748);
the drawn paths' mean length is in the file (mean_len_k{K}).
Both alternatives are checked for equality with the kernel before anything is timed.

Cold, as bench.py measures and as profiles/bench_swor.py does: ROTATE copies of the inputs are resident and take turns.
The kernel's calls are timed ITERS times with CUDA events around them and host wall time to the end of a synchronise;
the alternatives, which take up to seconds, ALT_ITERS times; medians.  The largest host cases run on the first
HOST_LATTICES lattices only and say so (``lattices`` in their entry): the work is per lattice."""
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfst_amd import decoders, ops, swor, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "20"))
ALT_ITERS = int(os.environ.get("ALT_ITERS", "3"))
BATCHES = os.environ.get("BATCHES", "baseline_b256,snips_b64").split(",")  # (a subset: the file keeps the other batch's entry)
ROTATE = int(os.environ.get("ROTATE", "4"))
HOST_THREADS = int(os.environ.get("HOST_THREADS", "16"))
HOST_LATTICES = int(os.environ.get("HOST_LATTICES", "16"))
HOST_CELLS = 2e9  # a host case above this many cells runs on HOST_LATTICES lattices
KS = (1, 16, 64)
dev = torch.device("cuda")


def timed(fns, iters):
    """fns: one callable per resident copy; call k runs fns[k % len(fns)]."""
    for f in (fns if iters >= len(fns) else fns[:1]):  # (every copy when the window uses them all; the slow alternatives once)
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
    return {"event_ms": round(statistics.median(ev), 4), "wall_ms": round(statistics.median(wall), 4), "iters": iters}


# ----------------------------------------------------------------------------- (a) the torch composition
def torch_edit_distance(a, al, b, bl):
    """[B, Ka, Kb] int32 by one row sweep over all pairs at once"""
    B, Ka, La = a.shape
    Kb, Lb = b.shape[1], b.shape[2]
    x = a[:, :, None, :].expand(B, Ka, Kb, La).reshape(-1, La)
    xl = al[:, :, None].expand(B, Ka, Kb).reshape(-1)
    y = b[:, None, :, :].expand(B, Ka, Kb, Lb).reshape(-1, Lb)
    yl = bl[:, None, :].expand(B, Ka, Kb).reshape(-1)
    col = torch.arange(Lb + 1, dtype=torch.int32, device=a.device)
    prev = col[None, :].repeat(x.shape[0], 1)
    for i in range(1, int(al.max()) + 1):
        t = torch.minimum(prev[:, 1:] + 1, prev[:, :-1] + (y != x[:, i - 1, None]))
        t = torch.cat((torch.full_like(t[:, :1], i), t), dim=1)
        d = torch.cummin(t - col, dim=1).values + col
        prev = torch.where((i <= xl)[:, None], d, prev)
    return prev.gather(1, yl.long()[:, None]).reshape(B, Ka, Kb)


# ----------------------------------------------------------------------------- (b) the host
def _host_set(x, xl, y, yl, symmetric):
    """[Ka, Kb] of one lattice: the same sweep in NumPy (int16) over its pairs, in symmetric mode over i < j only"""
    Ka, Kb = len(x), len(y)
    if symmetric:
        ii, jj = np.triu_indices(Ka, 1)
    else:
        ii, jj = (v.reshape(-1) for v in np.meshgrid(np.arange(Ka), np.arange(Kb), indexing="ij"))
    out = np.zeros((Ka, Kb), np.int32)
    if len(ii) == 0:
        return out
    m = int(yl.max())
    X, Xl, Y, Yl = x[ii], xl[ii], y[jj][:, :m], yl[jj]
    col = np.arange(m + 1, dtype=np.int16)
    prev = np.broadcast_to(col, (len(ii), m + 1)).copy()
    t = np.empty_like(prev)
    for i in range(1, int(Xl.max()) + 1):
        live = i <= Xl
        t[:, 0] = i
        np.minimum(prev[:, 1:] + np.int16(1), prev[:, :-1] + (Y != X[:, i - 1, None]).astype(np.int16), out=t[:, 1:])
        t -= col
        np.minimum.accumulate(t, axis=1, out=t)
        t += col
        if live.all():
            prev, t = t, prev
        else:
            prev[live] = t[live]
    d = prev[np.arange(len(ii)), Yl]
    out[ii, jj] = d
    if symmetric:
        out[jj, ii] = d
    return out


def host_edit_distance(a, al, b, bl, symmetric, pool, n_lat):
    """The copy to the host, then one task per lattice on the pool"""
    a, al, b, bl = (v[:n_lat].cpu().numpy() for v in (a, al, b, bl))
    return np.stack(list(pool.map(lambda s: _host_set(a[s], al[s], b[s], bl[s], symmetric), range(len(a)))))


# ----------------------------------------------------------------------------- one batch
def measure(name, lats, theta_np, pool, save):
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(theta_np).to(dev)
    B = lat.n_lattices
    g = swor.sample(lat, theta, 1, seed=2)
    gold, gold_len = g.paths[:, 0].contiguous(), g.lengths[:, 0].contiguous()
    r = {"lattices": B, "max_depth": int(lat.depth.max()), "rotate": ROTATE, "host_threads": HOST_THREADS}
    for k in KS:
        draw = swor.sample(lat, theta, k, seed=1)
        paths, lens = draw.paths, draw.lengths
        L = lens.double()
        r[f"mean_len_k{k}"] = round(float(L[L > 0].mean()), 1)
        cells_gold = float((L * gold_len.double()[:, None]).sum())
        cells_pair = float(((L.sum(1) ** 2 - (L ** 2).sum(1)) / 2).sum())
        sets = [(paths.clone(), lens.clone(), gold.clone(), gold_len.clone()) for _ in range(ROTATE)]
        draws = [draw._replace(paths=p, lengths=l) for p, l, _, _ in sets]

        # equality first
        D, P = ops.edit_distance(paths, lens, gold, gold_len), ops.pairwise_edit_distance(paths, lens)
        assert torch.equal(torch_edit_distance(paths, lens, gold[:, None], gold_len[:, None])[:, :, 0], D), (name, k)
        assert torch.equal(torch_edit_distance(paths, lens, paths, lens), P), (name, k)
        n_gold = B if cells_gold <= HOST_CELLS else min(B, HOST_LATTICES)
        n_pair = B if cells_pair <= HOST_CELLS else min(B, HOST_LATTICES)
        assert np.array_equal(host_edit_distance(paths, lens, gold[:, None], gold_len[:, None], False, pool, n_gold)[:, :, 0],
                              D[:n_gold].cpu().numpy()), (name, k)
        assert np.array_equal(host_edit_distance(paths, lens, paths, lens, True, pool, n_pair), P[:n_pair].cpu().numpy()), (name, k)
        risk = decoders.mbr_decode(draw)[1]

        def host_mbr(d, n):
            P_h = torch.from_numpy(host_edit_distance(d.paths, d.lengths, d.paths, d.lengths, True, pool, n))
            return decoders.mbr_select(P_h, swor.log_weights(d)[:n].cpu(), d.n_paths[:n].cpu())

        # (the distances are equal; the risks are float64 sums taken on two devices, and near-tied candidates may swap)
        assert torch.allclose(host_mbr(draw, n_pair)[1], risk[:n_pair].cpu(), rtol=1e-9, atol=1e-9), (name, k)

        e = r[f"gold_k{k}"] = timed([(lambda s=s: ops.edit_distance(*s)) for s in sets], ITERS)
        e["cells"], e["gcells_per_s"] = cells_gold, round(cells_gold / e["event_ms"] / 1e6, 2)
        r[f"gold_k{k}_torch"] = timed([(lambda s=s: torch_edit_distance(s[0], s[1], s[2][:, None], s[3][:, None])) for s in sets], ALT_ITERS)
        e = r[f"gold_k{k}_host"] = timed([(lambda s=s: host_edit_distance(s[0], s[1], s[2][:, None], s[3][:, None], False, pool, n_gold))
                                          for s in sets], ALT_ITERS)
        e["lattices"] = n_gold
        e = r[f"pairwise_k{k}"] = timed([(lambda s=s: ops.pairwise_edit_distance(s[0], s[1])) for s in sets], ITERS)
        e["cells"], e["gcells_per_s"] = cells_pair, round(cells_pair / e["event_ms"] / 1e6, 2)
        r[f"pairwise_k{k}_torch"] = timed([(lambda s=s: torch_edit_distance(s[0], s[1], s[0], s[1])) for s in sets], ALT_ITERS)
        e = r[f"pairwise_k{k}_host"] = timed([(lambda s=s: host_edit_distance(s[0], s[1], s[0], s[1], True, pool, n_pair)) for s in sets],
                                              ALT_ITERS)
        e["lattices"] = n_pair
        r[f"mbr_k{k}"] = timed([(lambda d=d: decoders.mbr_decode(d)) for d in draws], ITERS)
        r[f"mbr_k{k}_torch"] = timed([(lambda d=d: decoders.mbr_select(torch_edit_distance(d.paths, d.lengths, d.paths, d.lengths),
                                                                        swor.log_weights(d), d.n_paths)) for d in draws], ALT_ITERS)
        e = r[f"mbr_k{k}_host"] = timed([(lambda d=d: host_mbr(d, n_pair)) for d in draws], ALT_ITERS)
        e["lattices"] = n_pair
        print(name, k, json.dumps({key: v for key, v in r.items() if key.endswith(f"k{k}") or f"k{k}_" in key}), flush=True)
        save(name, r)  # (what is measured so far survives a run that is cut short)
    return r


def main():
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "edit.json"))
    out = {}
    if os.path.exists(path) and len(BATCHES) < 2:
        with open(path) as f:
            out = json.load(f)
    out.update({"device": torch.cuda.get_device_name(0), "iters": ITERS, "alt_iters": ALT_ITERS})

    def save(name, r):
        out[name] = r
        with open(path, "w") as f:
            json.dump(out, f, indent=1)

    with ThreadPoolExecutor(HOST_THREADS) as pool:
        if "baseline_b256" in BATCHES:
            measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256), pool, save)
        if "snips_b64" in BATCHES:
            measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8), pool, save)


if __name__ == "__main__":
    main()
