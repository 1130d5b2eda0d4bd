"""Bit equality of the tile-wave step against another build of the library ("Idle issue slots of the
sweep chain"; profiles/sweep_slots.json).

    python profiles/tune/sweep_slots_bits.py run OUT.json     one process = one library: the tree's own, or with
                                                              NFST_TUNING=1 NFST_LIB=<parent's libnfst_hip.so> the parent's
    python profiles/tune/sweep_slots_bits.py merge OUT.json parent=RUN.json new=RUN.json

``run`` hashes the raw bytes of every output of ``forward_backward`` (logz64, logalpha, logbeta, beta_me, posterior) and
``backward`` (logz64, logbeta, beta_me) under the default plan and under ``precise=1`` over the batches of
profiles/tune/tile_wave_sweep.py (those of tests/test_gpu_tile_wave_edges.py, a BASELINE-shaped batch, 300 deep chains) and
the inputs of tests/test_gpu_sweep_slots.py; for the latter it also counts the outputs of ``forward_backward`` on which
the float32 tile-wave kernel (``precise=0``) and the loader + decoder + sweep pipeline (``precise=0, tw=0``) disagree.
``merge`` counts the arrays that differ between the two libraries and writes both into OUT.json under "bits".
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
FB = ("logz64", "logalpha", "logbeta", "beta_me", "posterior")


def slot_batches(dev):
    """the inputs of tests/test_gpu_sweep_slots.py"""
    import torch
    from nfst_amd import synth
    from nfst_amd.lattice import LatticeBatch
    import test_gpu_sweep_slots as S

    mix = S.mixed_degree_lattice()
    lat = LatticeBatch.from_synth([mix], device=dev)
    thetas = [("seed1", S.mix_theta(1)), ("seed2", S.mix_theta(2))]
    thetas += [(f"low{k}", S.mix_theta(3, low_level=k)) for k in (1, 3, 4)]
    thetas += [(f"dead{k}", S.mix_theta(4, dead_label=S.level_labels(k)[0])) for k in (2, 3)]
    for name, th in thetas:
        yield "slots/mix/" + name, lat, torch.from_numpy(th)
    lats = [S.tiny_chain(n) for n in range(1, 10)]
    yield "slots/tiles1to9", LatticeBatch.from_synth(lats, device=dev), torch.from_numpy(synth.label_scores(11, 24, mean=-1.0, std=1.0))
    lats = [S.tiny_chain(2 + (i % 5)) for i in range(12)] + [synth.layered_lattice(40 + i, n_states=30 + i, avg_degree=3.0, vocab=24, width=3, span=2)
                                                              for i in range(8)]
    yield "slots/alignment", LatticeBatch.from_synth(lats, device=dev), torch.from_numpy(synth.label_scores(12, 24, mean=-1.0, std=1.0))
    l = synth.layered_lattice(51, n_states=1900, avg_degree=12.5, vocab=64, width=16, span=4)
    yield "slots/remainder", LatticeBatch.from_synth([l], device=dev), torch.from_numpy(synth.label_scores(13, 64))
    n = S.largest_tile_wave_rows(40)
    for n_rows in (n, n + 1):
        l = synth.layered_lattice(52, n_states=n_rows - 1, avg_degree=3.0, vocab=40, width=24, span=3)
        yield f"slots/rows{n_rows}", LatticeBatch.from_synth([l], device=dev), torch.from_numpy(synth.label_scores(14, 40))


def run(out):
    import torch
    from nfst_amd import ops, _lib
    import tile_wave_sweep as W

    dev = torch.device("cuda:0")
    digest, disagree, flavour_pairs = {}, [], 0
    sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    def both_ops(name, lat, theta, asc):
        for plan, switches in (("default", {}), ("precise", dict(precise=1))):
            with _lib.tuning(**switches):
                f = ops.forward_backward(lat, theta, arc_scores=asc, want_me=True)
                b = ops.backward(lat, theta, arc_scores=asc, want_me=True)
                torch.cuda.synchronize()
            for k in FB:
                digest[f"{name}/{plan}/forward_backward.{k}"] = sha(getattr(f, k))
            for k in ("logz64", "logbeta", "beta_me"):
                digest[f"{name}/{plan}/backward.{k}"] = sha(getattr(b, k))

    for name, lat, theta, asc in W.batches(dev):
        both_ops(name, lat, theta, asc)
    for name, lat, theta in slot_batches(dev):
        both_ops(name, lat, theta, None)
        res = []
        for switches in (dict(precise=0), dict(precise=0, tw=0)):
            with _lib.tuning(**switches):
                f = ops.forward_backward(lat, theta, want_me=True)
                torch.cuda.synchronize()
            res.append({k: sha(getattr(f, k)) for k in FB})
        for k in FB:
            digest[f"{name}/float32/forward_backward.{k}"] = res[0][k]
            flavour_pairs += 1
            if res[0][k] != res[1][k]:
                disagree.append(f"{name}/{k}")
    json.dump({"lib": _lib.LIB_PATH, "digest": digest, "flavour_pairs": flavour_pairs, "flavours_disagree": disagree}, open(out, "w"), indent=1)
    print(os.path.basename(_lib.LIB_PATH), len(digest), "arrays;", flavour_pairs, "tile-wave / pipeline pairs,", len(disagree), "disagree")


def merge(out, tagged):
    runs = dict(t.split("=", 1) for t in tagged)
    par, new = json.load(open(runs["parent"])), json.load(open(runs["new"]))
    keys = sorted(par["digest"])
    assert sorted(new["digest"]) == keys
    differ = [k for k in keys if par["digest"][k] != new["digest"][k]]
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["bits"] = {"what": "raw bytes of forward_backward (logz64, logalpha, logbeta, beta_me, posterior) and backward (logz64, logbeta, beta_me), "
                           "default plan and precise=1 (the inputs of tests/test_gpu_sweep_slots.py also under precise=0), parent's library against the tree's",
                   "arrays_compared": len(keys), "arrays_differ": len(differ), "differ": differ,
                   "flavours_agree_on_parent": {"pairs": par["flavour_pairs"], "disagree": par["flavours_disagree"]},
                   "flavours_agree_on_new": {"pairs": new["flavour_pairs"], "disagree": new["flavours_disagree"]}}
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps({k: v for k, v in doc["bits"].items() if k != "what"}))
    return 0 if not differ else 1


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else merge(sys.argv[2], sys.argv[3:]))
