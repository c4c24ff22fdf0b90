"""Static instruction counts of the kernels that run the row-strip depthwise item (mbconv_front_kernel, mbconv_mid_kernel) per barrier
interval, from the device assembly of mkws_embed.hip -- tools/mid_isa_counts.py with the front kernel and a finer split of the vector
instructions, for one build or for two side by side:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-fast-math -ffp-contract=off -S --cuda-device-only -o embed.s mkws_embed.hip
    python tools/strip_isa_counts.py parent.s [new.s]

Per instantiation: registers, spills, and for every stretch between two workgroup barriers the number of MFMA, v_pk_fma, transcendental
(v_exp / v_rcp), other vector-ALU, LDS, vector-memory and s_and_saveexec instructions in the text (a loop body counts once, so the figures
say what a phase is made of, not how often it runs).  With two files the intervals are printed as parent -> new."""
import re
import sys

KERNELS = (("mbconv_front_kernel", r"_ZN4mkws19mbconv_front_kernelI(\w+?)EEvNS_9FrontArgsE"),
           ("mbconv_mid_kernel", r"_ZN4mkws17mbconv_mid_kernelI(\w+?)EEvNS_7MidArgsE"))
COLUMNS = ("MFMA", "pk_fma", "trans", "VALU", "LDS", "VMEM", "saveexec")


def count(part):
    ops = [ln.split()[0] for ln in part.splitlines() if ln.startswith("\t") and ln.strip() and not ln.startswith("\t.") and not ln.startswith("\t;")]
    mfma = sum(o.startswith("v_mfma") for o in ops)
    pk_fma = sum(o.startswith("v_pk_fma") for o in ops)
    trans = sum(o.startswith(("v_exp", "v_rcp")) for o in ops)
    valu = sum(o.startswith("v_") for o in ops) - mfma - pk_fma - trans
    lds = sum(o.startswith("ds_") for o in ops)
    vmem = sum(o.startswith(("buffer_", "global_", "flat_")) for o in ops)
    return (mfma, pk_fma, trans, valu, lds, vmem, sum(o.startswith("s_and_saveexec") for o in ops))


def kernels(path):
    """{display name: (header text, [counts per barrier interval])}"""
    text, out = open(path).read(), {}
    for kernel, pattern in KERNELS:
        for m in re.finditer(r"^(" + pattern + r"):.*$", text, re.M):
            name, args = m.group(1), m.group(2)
            end = text.index(".Lfunc_end", m.end())
            meta = {k: re.search(r"; %s: (\d+)" % k, text[end:]).group(1) for k in ("NumVgprs", "ScratchSize", "Occupancy")}
            spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", text[text.index(".name:           " + name):]).group(1)
            params = ",".join(re.findall(r"L[ib](\d+)E", args))
            head = f"VGPRs {meta['NumVgprs']}, spilled {spill}, scratch {meta['ScratchSize']} B, occupancy {meta['Occupancy']} waves/SIMD"
            out[f"{kernel}<{params}>"] = (head, [count(part) for part in text[m.end():end].split("s_barrier")])
    return out


def main():
    builds = [kernels(p) for p in sys.argv[1:3]]
    if not builds:
        sys.exit(__doc__)
    print("columns per interval: " + " / ".join(COLUMNS) + (";  parent -> new" if len(builds) == 2 else ""))
    for name, (head, rows) in builds[0].items():
        if len(builds) == 1:
            print(f"{name}: {head}")
            for k, row in enumerate(rows):
                print(f"  interval {k:2d}: " + " ".join(f"{v:4d}" for v in row))
            continue
        head2, rows2 = builds[1].get(name, ("absent", []))
        print(f"{name}:\n  parent {head}\n  new    {head2}")
        for k in range(max(len(rows), len(rows2))):
            a = " ".join(f"{v:4d}" for v in rows[k]) if k < len(rows) else "-"
            b = " ".join(f"{v:4d}" for v in rows2[k]) if k < len(rows2) else "-"
            print(f"  interval {k:2d}: {a}  ->  {b}")
        if rows and rows2:
            ta, tb = [sum(r[i] for r in rows) for i in range(len(COLUMNS))], [sum(r[i] for r in rows2) for i in range(len(COLUMNS))]
            print("  whole text : " + " ".join(f"{v:4d}" for v in ta) + "  ->  " + " ".join(f"{v:4d}" for v in tb))


if __name__ == "__main__":
    main()
