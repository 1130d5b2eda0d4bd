"""Issue slots of the tile waves' three-tile trip (WeightWave<8, 4, .., FULL>::run_tiles), counted in the library's code
object (no GPU needed; DESIGN.md section 4.1, "The tile-wave loop on a diet"; profiles/tile_wave_diet.json).

    python profiles/tune/tile_wave_slots.py [LIB.so] [--tag TAG] [--json OUT.json] [--dump]

Uses the disassembly and loop finding of trip_slots.py.  In each kernel named below a tile-wave loop is an innermost
loop that holds global loads -- three tiles' worth at least -- and ds_write_b128 and no cross-lane (DPP) instruction.
A kernel that chooses the ring format in front of the loop has one loop per format, and both are printed under the
format's name: ``narrow`` (the decoded tile of tile_sweep2, which the benchmark runs: the only per-lane ds_write_b32 is
the wave's flag, one per tile) and ``wide`` (a control word per lane besides); a loop that holds both formats behind
branches (the code before the diet) is ``both``.  Per loop: the instruction classes of trip_slots.py, ``issued``
(everything but the waits), ``per_tile`` (a trip is three tiles) and the mnemonics that occur more than three times.
``--json`` appends the result under TAG to OUT.json, with the kernels' register counts from the resource report beside
the library.  The tool only counts; it judges nothing.
"""
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trip_slots as ts  # noqa: E402

KERNELS = {
    "float32_preloaded": ("18k_forward_backwardILi1024ELi0ELb0ELb1ELb0ELb1EE", "k_forward_backward<1024, 0, false, true, false, true>"),
    "float32_grad_theta": ("18k_forward_backwardILi1024ELi0ELb0ELb1ELb0ELb0EE", "k_forward_backward<1024, 0, false, true, false, false>"),
    "precise": ("18k_forward_backwardILi1024ELi0ELb0ELb1ELb1ELb0EE", "k_forward_backward<1024, 0, false, true, true, false>"),
    "extra1": ("18k_forward_backwardILi1024ELi1ELb0ELb1ELb0ELb0EE", "k_forward_backward<1024, 1, false, true, false, false>"),
    "backward": ("10k_backwardILi512ELi0ELb1ELb0EE", "k_backward<512, 0, true, false>"),
}


def tile_wave_loops(code):
    out = []
    for j, i in ts.innermost_loops(code):
        body = code[j:i + 1]
        c = ts.classify(body)
        ops = collections.Counter(op for _, op, _ in body)
        loads = sum(v for k, v in ops.items() if k.startswith("global_load"))
        if c["dpp"] == 0 and loads >= 3 and ops["ds_write_b128"] > 0:
            w128, w32 = ops["ds_write_b128"], ops["ds_write_b32"]
            name = "both" if w128 > 15 else "narrow" if w32 <= 3 else "wide"
            out.append((name, c, body))
    return out


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    opt = lambda k: argv[argv.index(k) + 1] if k in argv else None
    for k in ("--tag", "--json"):
        if opt(k) in args:
            args.remove(opt(k))
    lib = args[0] if args else os.path.join(ts.ROOT, "nfst_amd", "lib", "libnfst_hip.so")
    fns = ts.functions(ts.disassemble(lib))
    res_path = lib[:-3] + ".resources.json"
    res = json.load(open(res_path)) if os.path.exists(res_path) else {}
    out = {}
    for tag, (frag, res_name) in KERNELS.items():
        sym = [s for s in fns if frag in s and not s.endswith(".kd")]
        if len(sym) != 1:
            raise SystemExit(f"{tag}: {len(sym)} symbols match {frag}")
        entry = {}
        for name, c, body in tile_wave_loops(fns[sym[0]]):
            c["per_tile"] = round(c["issued"] / 3.0, 2)
            ops = collections.Counter(op for _, op, _ in body)
            c["mnemonics"] = {k: v for k, v in sorted(ops.items(), key=lambda kv: -kv[1]) if v > 3}
            while name in entry:
                name += "_"
            entry[name] = c
            print(tag, name, json.dumps(c))
            if "--dump" in argv:
                for a, op, ar in body:
                    print("  %06x  %s %s" % (a, op, ar))
        r = next((v for k, v in res.items() if k.split("(")[0].strip() == res_name), None)
        if r is not None:
            entry["registers"] = {k: r.get(k) for k in ("vgprs", "agprs", "sgprs", "scratch", "vgpr_spill", "sgpr_spill", "occupancy")}
        out[tag] = entry
    if opt("--json"):
        path = opt("--json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.setdefault("tile_wave_loop", {})[opt("--tag") or "new"] = out
        json.dump(doc, open(path, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
