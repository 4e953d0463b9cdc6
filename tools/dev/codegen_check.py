"""development: instruction mix of a packed bundle kernel (catches register-copy blow-ups, SGPR spills and -- the one that
cost 9 % in round 3 -- FLAT loads in the main loop: every load must be global_load or s_load)
usage: codegen_check.py <method nw|ga|sw> [G = 8|16] [KLO = 9] [f16 = 1] [-DMACRO=VALUE ...]
NW also prints the body of one step per K of the bundle (the instructions between two DPP moves that hold exactly K
v_pk_maximum3_f16 -- the K = 14 row is the step cfg 2 spends its time in): VALU, s_nop, 64-bit adds, register copies, waits"""
import collections, pathlib, re, subprocess, sys
defs = [a for a in sys.argv[1:] if a.startswith("-D")]
argv = [a for a in sys.argv[1:] if not a.startswith("-D")]
m = argv[0] if len(argv) > 0 else "nw"
g = int(argv[1]) if len(argv) > 1 else 8
klo = int(argv[2]) if len(argv) > 2 else (9 if g == 8 else 13)
f16 = int(argv[3]) if len(argv) > 3 else 1
mi = {"nw": 0, "ga": 1, "sw": 2}[m]
tu = f"sa_systolic_pk_{m}.hip" if g == 8 else f"sa_systolic_pk16{'hi' if klo >= 45 else ''}_{m}.hip"
csrc = pathlib.Path(__file__).resolve().parents[2] / "sequencealigner_amd" / "csrc"
asm = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-x", "hip", "--cuda-device-only",
                      *defs, "-S", str(csrc / tu), "-o", "-"], capture_output=True, text=True).stdout
name = f"_ZN12_GLOBAL__N_123sa_k_systolic_pk_bundleILi{mi}ELi{g}ELi{klo}ELb{f16}EEEv9SaSysArgs"
body = asm[asm.index(name + ":"):]
tail = body[body.index("s_endpgm"):]
body = body[:body.index("s_endpgm")]
ops = [l.split()[0] for l in body.split("\n") if l.strip() and not l.strip().startswith((";", ".")) and not l.strip().endswith(":")]
c = collections.Counter(ops)
print(name, *defs)
print("instructions", len(ops))
for k in ("flat_load_ubyte", "flat_load_dword", "global_load_ubyte", "global_load_dword", "s_load_dword", "v_readlane_b32", "v_writelane_b32",
          "v_readfirstlane_b32", "v_pk_maximum3_f16", "v_pk_max_u16", "v_add_u32_e32", "v_lshl_add_u64", "v_sub_u32_e32", "v_mov_b32_e32", "v_mov_b32_dpp",
          "ds_read_b128", "ds_read_u16", "s_nop", "s_waitcnt", "s_setprio"):
    print(f"  {k:22s} {c.get(k, 0)}")
flat = sum(v for k, v in c.items() if k.startswith("flat_"))
print("FLAT memory instructions:", flat, "(must be 0)" if flat else "")
for key in ("codeLenInByte", "ScratchSize"):
    mm = re.search(r"; " + key + r"\s*[=:]\s*(\d+)", tail)
    print(key, mm.group(1) if mm else "?")
for key in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count"):
    for mm in re.finditer(r"\.name:\s+" + name + r"\n(?:.*\n)*?\s+\." + key + r":\s+(\d+)", asm):
        print(key, mm.group(1))
if m == "nw" and f16:
    # a NW step has ONE DPP move (the left neighbour's value) in front of its K maxima: cut the kernel at the DPP moves and
    # keep, per K, the most frequent shape among the pieces with exactly K maxima (15 of the 16 steps of a block)
    cuts = [i for i, o in enumerate(ops) if o == "v_mov_b32_dpp"]
    shapes = collections.defaultdict(collections.Counter)
    valus = collections.defaultdict(collections.Counter)
    for a, b in zip(cuts, cuts[1:]):
        sc = collections.Counter(ops[a:b])
        valus[sc["v_pk_maximum3_f16"]][sum(v for o, v in sc.items() if o.startswith("v_"))] += 1
        shapes[sc["v_pk_maximum3_f16"]][(b - a, sum(v for o, v in sc.items() if o.startswith("v_")), sc["s_nop"], sc["v_lshl_add_u64"],
                                         sc["v_mov_b32_e32"], sc["s_waitcnt"])] += 1
    print("step body per K (most frequent of the steps found): instructions, VALU, s_nop, v_lshl_add_u64, v_mov_b32, s_waitcnt")
    for k in range(klo, klo + 8):
        if shapes.get(k):
            (n, valu, nop, add64, mov, wait), cnt = shapes[k].most_common(1)[0]
            print(f"  K = {k:2d}: {n:3d} instructions, {valu:2d} VALU, s_nop {nop:2d}, v_lshl_add_u64 {add64}, v_mov_b32 {mov}, s_waitcnt {wait}   ({cnt} steps of this shape)")
            # a piece that runs from the last step of a block into the first of the next carries that block's work outside the
            # steps: its VALU count less the plain step's (the main loop is two blocks per way; cold event paths lie elsewhere)
            print("          VALU of every piece with K maxima (VALU: pieces):", ", ".join(f"{v}: {n}" for v, n in sorted(valus[k].items())))
