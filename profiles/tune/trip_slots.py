"""Issue slots of the four-tile trip of tile_sweep2, counted in the library's code object (no GPU needed; DESIGN.md
section 4.1, "Idle issue slots of the sweep chain"; profiles/sweep_slots.json).

    python profiles/tune/trip_slots.py [LIB.so] [--tag TAG] [--json OUT.json] [--dump]

Unbundles the gfx950 code object of LIB.so (default: the tree's own library), disassembles it and, for the float32
kernel with preloaded label weights (``k_forward_backward<1024, 0, false, true, false, true>``) and the precise one
(``<1024, 0, false, true, true, false>``), finds the trip: among the kernel's innermost loops (a backward branch and its
target with no other backward branch between them) the one with the most cross-lane (DPP) stages -- the segmented
sums of four tiles.  It prints the trip's instructions by class:

    valu       vector ALU (the scalar-to-vector moves below are counted apart)
    s2v_moves  v_mov_b32 of a scalar register into a vector register
    salu       scalar ALU, branches included
    lds        ds_*
    vmem       global_* / buffer_* / flat_*
    nops       s_nop (wait states written by hand or put there by the compiler's hazard recogniser)
    waits      s_waitcnt, and how many of them wait for a counter to reach zero ("full")

``issued`` = everything but the waits.  ``--json`` appends the result under TAG to OUT.json (with the kernels' register
counts from the resource report beside the library, where there is one); ``--dump`` prints the trip's text.
The tool only counts; it judges nothing.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
KERNELS = {"float32_preloaded": "18k_forward_backwardILi1024ELi0ELb0ELb1ELb0ELb1EE",
           "precise": "18k_forward_backwardILi1024ELi0ELb0ELb1ELb1ELb0EE"}
RES_NAMES = {"float32_preloaded": "k_forward_backward<1024, 0, false, true, false, true>",
             "precise": "k_forward_backward<1024, 0, false, true, true, false>"}


def disassemble(lib):
    with tempfile.TemporaryDirectory() as d:
        co, fat = os.path.join(d, "gfx950.co"), os.path.join(d, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                              capture_output=True, text=True).stdout


def functions(text):
    """{symbol: [(address, mnemonic, operands)]}"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return out


def branch_target(ins, labels):
    a, op, args = ins
    if not op.startswith("s_cbranch") and op != "s_branch":
        return None
    m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", args)
    if m:
        return labels["base"] + int(m.group(1), 16)
    m = re.match(r"^(-?\d+)$", args.strip())
    if m:  # a raw word offset relative to the next instruction
        off = int(m.group(1))
        if off >= 0x8000:
            off -= 0x10000
        return a + 4 + 4 * off
    return None


def innermost_loops(code):
    labels = {"base": code[0][0]}
    back = []
    for i, ins in enumerate(code):
        t = branch_target(ins, labels)
        if t is not None and t <= ins[0]:
            back.append((t, i))
    addr_index = {a: i for i, (a, _, _) in enumerate(code)}
    loops = []
    for t, i in back:
        if t not in addr_index:
            continue
        j = addr_index[t]
        if not any(j <= k < i for _, k in back if k != i):
            loops.append((j, i))
    return loops


def classify(body):
    c = {"valu": 0, "s2v_moves": 0, "salu": 0, "lds": 0, "vmem": 0, "nops": 0, "waits": 0, "full_waits": 0, "dpp": 0, "lines": len(body)}
    for _, op, args in body:
        if op == "s_waitcnt":
            c["waits"] += 1
            if re.search(r"cnt\(0\)", args):
                c["full_waits"] += 1
        elif op == "s_nop":
            c["nops"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("v_"):
            ops = [a.strip() for a in args.split(",")]
            if op.startswith("v_mov_b32") and "dpp" not in op and len(ops) == 2 and re.match(r"^s\d+$", ops[1]):
                c["s2v_moves"] += 1
            else:
                c["valu"] += 1
            if "dpp" in op or "quad_perm" in args or "row_" in args:
                c["dpp"] += 1
        else:
            c["salu"] += 1
    c["issued"] = c["lines"] - c["waits"]
    return c


def trip_of(code):
    best = None
    for j, i in innermost_loops(code):
        body = code[j:i + 1]
        c = classify(body)
        if best is None or c["dpp"] > best[0]["dpp"]:
            best = (c, body)
    return best


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    opt = lambda k: argv[argv.index(k) + 1] if k in argv else None
    for k in ("--tag", "--json"):
        if opt(k) in args:
            args.remove(opt(k))
    lib = args[0] if args else os.path.join(ROOT, "nfst_amd", "lib", "libnfst_hip.so")
    fns = functions(disassemble(lib))
    res_path = lib[:-3] + ".resources.json"
    res = json.load(open(res_path)) if os.path.exists(res_path) else {}
    out = {}
    for tag, frag in KERNELS.items():
        sym = [s for s in fns if frag in s and not s.endswith(".kd")]
        if len(sym) != 1:
            raise SystemExit(f"{tag}: {len(sym)} symbols match {frag}")
        c, body = trip_of(fns[sym[0]])
        c["per_tile"] = round(c["issued"] / 4.0, 2)
        r = next((v for k, v in res.items() if k.split("(")[0].strip() == RES_NAMES[tag]), None)
        if r is not None:
            c["registers"] = {k: r.get(k) for k in ("vgprs", "agprs", "sgprs", "scratch", "vgpr_spill", "sgpr_spill", "occupancy")}
        out[tag] = c
        print(tag, json.dumps(c))
        if "--dump" in argv:
            for a, op, ar in body:
                print("  %06x  %s %s" % (a, op, ar))
    if opt("--json"):
        path = opt("--json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.setdefault("trip", {})[opt("--tag") or "new"] = out
        json.dump(doc, open(path, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
