"""One step of lattice-constrained beam search: the fused nfst_beam_step next to the same step
composed from the ops the engine had before it.  Writes profiles/beam.json, per K in (16, 64) on B = 32 lattices of
the BASELINE shape (synth.bench_batch(32), vocabulary 256):

  beam_step        ops.beam_step into output buffers allocated once (one launch)
  composed         ops.emission_mask + (beam_score + (scores with the pad column at zero + mask)) + torch.topk over
                   K * V per lattice + parent / symbol from the flat index + ops.step: the same survivors' scores
    mask / add_topk / step   its parts alone

The slots are those of a search in progress: WARM steps of the beam under random log-probabilities, so that every
slot is live and the slots of a lattice sit in different states.  A step of a decoding loop runs on data the step before
it has just touched, so the calls are timed warm: CALLS back-to-back calls between two events, the time per call is the
window over CALLS, the median of ITERS windows is reported (GPU time incl. the gaps between launches; the host keeps
ahead of the device for the fused step and is part of the composed one's time where its launches are short)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import ops, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "15"))
CALLS = int(os.environ.get("CALLS", "200"))
WARM = 12
B = 32
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
dev = torch.device("cuda")


def per_call_us(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(ITERS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(CALLS):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / CALLS)
    return {"us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def measure(lat, K):
    V, N = lat.vocab, B * K
    g = torch.Generator(device="cpu").manual_seed(K)
    scores = torch.log_softmax(torch.randn(N, V, generator=g), dim=1).to(dev)
    inp = torch.full((N,), BOS, dtype=torch.int64, device=dev)
    state = ops.step(lat, torch.zeros(N, dtype=torch.int64, device=dev), inp, k=K)
    score = torch.full((N,), float("-inf"), device=dev)
    score[::K] = 0.0
    for _ in range(WARM):
        r = ops.beam_step(lat, state, inp, score, scores, K, pad=PAD, bos=BOS, eos=EOS)
        state, inp, score = r.next_state, r.symbol, r.score
    live = int((score > float("-inf")).sum())
    out = tuple(torch.empty_like(x) for x in r)
    fused = lambda: ops.beam_step(lat, state, inp, score, scores, K, pad=PAD, bos=BOS, eos=EOS, out=out)
    base = (torch.arange(N, device=dev) // K * K)

    def mask():
        return ops.emission_mask(lat, state, k=K, inp=inp, pad=PAD, bos=BOS, eos=EOS)

    sc0 = scores.clone()
    sc0[:, PAD] = 0.0

    def add_topk(m):
        cand = score[:, None] + (sc0 + m)
        return torch.topk(cand.view(B, K * V), K, dim=1)

    def step(top):
        flat = top.indices.reshape(-1)
        parent, symbol = flat // V, flat % V
        return ops.step(lat, state[base + parent], symbol, k=K), parent, symbol

    def composed():
        top = add_topk(mask())
        return top.values, step(top)

    m0 = mask()
    t0 = add_topk(m0)
    got = fused()
    torch.cuda.synchronize()
    same = bool(torch.equal(got.score.view(B, K), t0.values))  # (untied inputs: the same survivors' scores)
    res = {"slots": N, "live_slots": live, "candidates_per_lattice_mean": round(float(got.n_candidates.float().mean()), 1),
           "same_scores_as_composed": same, "beam_step": per_call_us(fused), "composed": per_call_us(composed),
           "composed_parts": {"mask": per_call_us(mask), "add_topk": per_call_us(lambda: add_topk(m0)), "step": per_call_us(lambda: step(t0))}}
    res["ratio_beam_step_over_composed"] = round(res["beam_step"]["us"] / res["composed"]["us"], 3)
    print(K, json.dumps(res), flush=True)
    return res


def main():
    lat = LatticeBatch.from_synth(synth.bench_batch(B), device=dev)
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS, "calls_per_window": CALLS, "lattices": B, "vocab": lat.vocab,
           "rows": int(lat.total_rows), "arcs": int(lat.total_arcs), "warm_steps": WARM}
    for K in (16, 64):
        out[f"k{K}"] = measure(lat, K)
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "beam.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
