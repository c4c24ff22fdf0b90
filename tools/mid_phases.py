"""Phase table of mbconv_mid_kernel from the timing build (make -C multilingual_kws_amd/csrc timing).

    python tools/mid_phases.py [--lib PATH/libmkws_hip_timing.so] [--clips 1024] [--passes 9] [--label TEXT]

Runs tools/one_fwd.py (--passes forward passes) in a child process on that library, drops the first pass as warm-up and prints, per
whole-block launch, the mean over the remaining passes of every figure on the kernel's [mid-timing] and [mid-phases] lines:
thread 0's wall-clock time per phase, averaged over the workgroups (the slots are listed at MID_STAMP in mkws_embed.hip)."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM = re.compile(r"-?\d+\.\d+")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "multilingual_kws_amd", "lib", "libmkws_hip_timing.so"))
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    env = dict(os.environ, MKWS_LIB=os.path.abspath(args.lib), ONE_FWD_B=str(args.clips), ONE_FWD_PASSES=str(args.passes))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "one_fwd.py")], env=env, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, timeout=600)
    if run.returncode != 0:
        sys.stderr.write(run.stderr[-4000:])
        sys.exit(run.returncode)
    rows = {}                                     # (tag, stage) -> [text with the figures cut out, [figures of each launch]]
    for line in run.stderr.splitlines():
        m = re.match(r"\[(mid-timing|mid-phases)\] (\S+?):? (.*)", line)
        if not m:
            continue
        tag, stage, rest = m.groups()
        rows.setdefault((tag, stage), [NUM.sub("{}", rest), []])[1].append([float(v) for v in NUM.findall(rest)])
    if not rows:
        sys.exit("no [mid-timing] lines: is --lib a timing build?")
    print(f"# {args.label or args.lib}: {args.clips} clips, mean of the launches after the first")
    for (tag, stage), (text, runs) in rows.items():
        kept = runs[1:] or runs
        mean = [sum(r[i] for r in kept) / len(kept) for i in range(len(kept[0]))]
        print(f"[{tag}] {stage} ({len(kept)} launches): " + text.format(*[f"{v:.2f}" for v in mean]))


if __name__ == "__main__":
    main()
