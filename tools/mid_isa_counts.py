"""Static instruction counts of mbconv_mid_kernel per barrier interval, from the device assembly of mkws_embed.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-fast-math -ffp-contract=off -S --cuda-device-only -o embed.s mkws_embed.hip
    python tools/mid_isa_counts.py embed.s

Per instantiation: registers, scratch, and for every stretch between two workgroup barriers the number of MFMA, other vector-ALU, LDS and
vector-memory instructions in the text (a loop body counts once, so the figures say what a phase is made of, not how often it runs)."""
import re
import sys


def main():
    text = open(sys.argv[1]).read()
    for m in re.finditer(r"^(_ZN4mkws17mbconv_mid_kernelI(\w+?)EEvNS_7MidArgsE):.*$", text, re.M):
        name, args = m.group(1), m.group(2)
        body = text[m.end():text.index(".Lfunc_end", m.end())]
        tail = text[text.index(".Lfunc_end", m.end()):]
        meta = {k: re.search(r"; %s: (\d+)" % k, tail).group(1) for k in ("NumVgprs", "ScratchSize", "Occupancy")}
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", text[text.index(".name:           " + name):]).group(1)
        params = [int(v) for v in re.findall(r"L[ib](\d+)E", args)]
        print(f"mbconv_mid_kernel<{','.join(map(str, params))}>: VGPRs {meta['NumVgprs']}, spilled {spill}, scratch {meta['ScratchSize']} B, occupancy {meta['Occupancy']} waves/SIMD")
        for k, part in enumerate(body.split("s_barrier")):
            ops = [ln.split()[0] for ln in part.splitlines() if ln.startswith("\t") and ln.strip() and not ln.startswith("\t.") and not ln.startswith("\t;")]
            mfma = sum(o.startswith("v_mfma") for o in ops)
            valu = sum(o.startswith("v_") for o in ops) - mfma
            lds = sum(o.startswith("ds_") for o in ops)
            vmem = sum(o.startswith(("buffer_", "global_", "flat_")) for o in ops)
            print(f"  interval {k:2d}: MFMA {mfma:3d}  VALU {valu:4d}  LDS {lds:3d}  VMEM {vmem:3d}")


if __name__ == "__main__":
    main()
