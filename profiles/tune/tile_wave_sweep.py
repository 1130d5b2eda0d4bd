"""Bit equality and float64-flavour timing of the tile-wave sweep against another build of the library (DESIGN.md
section 4.1, "One sweep loop for both value types"; profiles/tile_wave_sweep.json).

    python profiles/tune/tile_wave_sweep.py run OUT.json          one process = one library: the tree's own, or with
                                                                  NFST_TUNING=1 NFST_LIB=<parent's libnfst_hip.so> the parent's
    python profiles/tune/tile_wave_sweep.py merge OUT.json TAG=RUN.json ...     TAG: parent or new, in the order they ran

``run`` writes a SHA-256 of the raw bytes of every output of ``forward_backward`` (logz64, logalpha, logbeta, beta_me,
posterior) and ``backward`` (logz64, logbeta, beta_me) under the default plan and under ``precise=1``, over the batches of
tests/test_gpu_tile_wave_edges.py, one BASELINE-shaped batch and 300 chains of 300 levels; and the time of
``forward_backward`` under ``precise=1`` on the last batch by HIP events.  ``merge`` counts the arrays that differ between
the parent's runs and the new ones (an array on which the parent's own runs disagree is left out and counted as such)
and puts the timings side by side: the new runs must not be slower than the parent's slowest run.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def batches(dev):
    import numpy as np
    import torch
    from nfst_amd import synth
    from nfst_amd.lattice import LatticeBatch
    import test_gpu_tile_wave_edges as E

    for bi, levels in enumerate(E.BATCHES):
        for ex in E.EXTRAS:
            lats = [E._chain(n, ex != "none", 100 * bi + i) for i, n in enumerate(levels)]
            theta = torch.from_numpy(synth.label_scores(7 + bi, E.V, mean=-1.0, std=1.0))
            for gm in (0, 2):
                lat = LatticeBatch.from_synth(lats, device=dev, group_mode=gm)
                asc = None
                if ex == "weights+scores":
                    asc = torch.from_numpy(np.random.default_rng(50 + bi).normal(0.0, 0.5, size=lat.total_arcs).astype(np.float32))
                yield f"edges{bi}/{ex}/gm{gm}", lat, theta, asc
    lats = synth.bench_batch(256, first_seed=1234, width=16)
    yield "baseline256", LatticeBatch.from_synth(lats, device=dev), torch.from_numpy(synth.label_scores(0, lats[0].vocab)), None
    yield deep_chains(dev)


def deep_chains(dev):  # the batch of test_precise_flavour_beyond_one_lattice_per_cu_and_through_autograd
    import torch
    from nfst_amd import synth
    from nfst_amd.lattice import LatticeBatch
    lats = [synth.layered_lattice(700 + i, n_states=300 + (i % 7), avg_degree=2.5, vocab=40, width=1, span=1 + i % 2, max_degree=6) for i in range(300)]
    lat = LatticeBatch.from_synth(lats, device=dev)
    asc = (torch.randn(lat.total_arcs, generator=torch.Generator().manual_seed(3)) * 0.3).to(dev)
    return "chains300x300", lat, torch.from_numpy(synth.label_scores(5, 40, mean=-1.0, std=1.0)), asc


def run(out):
    import torch
    from nfst_amd import ops, _lib

    dev = torch.device("cuda:0")
    digest = {}
    for name, lat, theta, asc in batches(dev):
        for plan, switches in (("default", {}), ("precise", dict(precise=1))):
            with _lib.tuning(**switches):
                f = ops.forward_backward(lat, theta, arc_scores=asc, want_me=True)
                b = ops.backward(lat, theta, arc_scores=asc, want_me=True)
                torch.cuda.synchronize()
            for op, r, fields in (("forward_backward", f, ("logz64", "logalpha", "logbeta", "beta_me", "posterior")),
                                  ("backward", b, ("logz64", "logbeta", "beta_me"))):
                for k in fields:
                    digest[f"{name}/{plan}/{op}.{k}"] = hashlib.sha256(getattr(r, k).cpu().numpy().tobytes()).hexdigest()
    # the float64 flavour's step: 300 lattices of 300 levels, windows of 50 back-to-back launches between two events
    _, lat, theta, asc = deep_chains(dev)
    theta = theta.to(dev)
    windows = []
    with _lib.tuning(precise=1):
        for w in range(3 + 9):  # (three windows of warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                ops.forward_backward(lat, theta, arc_scores=asc)
            e1.record()
            torch.cuda.synchronize()
            if w >= 3:
                windows.append(e0.elapsed_time(e1) * 1e3 / 50)
    windows.sort()
    json.dump({"lib": _lib.LIB_PATH, "digest": digest, "precise_fb_us_windows": [round(x, 3) for x in windows],
               "precise_fb_us": round(windows[len(windows) // 2], 3)}, open(out, "w"), indent=1)
    print(os.path.basename(_lib.LIB_PATH), len(digest), "arrays; precise forward_backward, 300 x 300 levels:", round(windows[len(windows) // 2], 2), "us")


def merge(out, tagged):
    runs = [(t.split("=", 1)[0], json.load(open(t.split("=", 1)[1]))) for t in tagged]
    par = [r for t, r in runs if t == "parent"]
    new = [r for t, r in runs if t == "new"]
    keys = sorted(par[0]["digest"])
    assert all(sorted(r["digest"]) == keys for _, r in runs)
    unstable = [k for k in keys if len({r["digest"][k] for r in par}) > 1]
    compared = [k for k in keys if k not in unstable]
    differ = [k for k in compared if any(r["digest"][k] != par[0]["digest"][k] for r in new)]
    pt, nt = [r["precise_fb_us"] for r in par], [r["precise_fb_us"] for r in new]
    res = {"arrays": len(keys), "compared_as_raw_bits": len(compared), "left_out_parent_disagrees_with_itself": unstable,
           "differ": differ, "plans": ["default", "precise=1"],
           "precise_forward_backward_us": {"what": "300 chains of 300 levels with caller scores, precise=1, median of 9 windows of 50 launches per run",
                                           "order": [t for t, _ in runs], "parent": pt, "new": nt,
                                           "new_within_parents_range": max(nt) <= max(pt)}}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "left_out_parent_disagrees_with_itself"}))
    return 0 if not differ else 1


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else merge(sys.argv[2], sys.argv[3:]))
