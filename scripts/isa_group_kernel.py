"""Static figures of score_group_kernel's pose instance (csrc/score.hip) from the gfx950 assembly the Makefile's flags give.
usage: python scripts/isa_group_kernel.py [-DPGX_SCORE_TRIM=<mask> ...] [--keep FILE] [--instance SUBSTRING]

Prints the instance's VGPRs, SGPRs and scratch, the number of s_waitcnt with lgkmcnt(0) between the kernel's entry and its first
global_load (the dependent scalar round trips a listed workgroup passes before its rows are requested, in layout order), and for
the innermost step block - the shortest backward-branch span that holds the survivor scan (s_ff1_i32_b64) and an LDS read - the
lines that begin with v_, ds_ and s_cbranch.  It counts by these prefixes and nothing else: a measuring aid for
docs/lab-notebook.md, not a test."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "progressive-x_amd", "csrc")
POSE = "score_group_kernelILi3ELb0ELb0EE"      # <kPnP, MASK = false, STATS = false>


def makefile_flags():
    """CXXFLAGS of csrc/Makefile with ARCH and EXTRA substituted (EXTRA comes from the command line)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= *(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS = *(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()


def assemble(extra, keep):
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC \?= *(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1))
    out = keep or os.path.join(tempfile.mkdtemp(prefix="isa_group_"), "score.s")
    subprocess.check_call([hipcc] + makefile_flags() + extra + ["--cuda-device-only", "-S", "-o", out, "score.hip"], cwd=CSRC)
    return open(out).read().splitlines()


def function_body(lines, name):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(name), l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".amdhsa_kernel"))
    info = next(i for i in range(end, len(lines)) if lines[i].startswith("; Kernel info:"))
    return lines[start + 1:end], lines[info:info + 20]


def scratch_of_every_instance(lines):
    """(instances, those with scratch) of score_group_kernel and score_cull_kernel, every model type"""
    n, bad, name = 0, [], None
    for l in lines:
        m = re.match(r"^(_Z\w*score_(?:group|cull)_kernel\w*):", l)
        if m:
            name = m.group(1)
        m = re.match(r"^; ScratchSize: (\d+)", l)
        if m and name:
            n += 1
            if int(m.group(1)):
                bad.append((name, int(m.group(1))))
            name = None
    return n, bad


def op(line):
    s = line.split(";")[0].strip()
    return s.split()[0] if s and not s.endswith(":") and not s.startswith(".") else ""


def step_block(body):
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    best = None
    for i, l in enumerate(body):
        o = op(l)
        if not (o.startswith("s_cbranch") or o == "s_branch"):
            continue
        tgt = labels.get(l.split(";")[0].split()[-1])
        if tgt is None or tgt > i:
            continue
        ops = [op(x) for x in body[tgt:i + 1]]
        if "s_ff1_i32_b64" in ops and any(x.startswith("ds_read") for x in ops) and (best is None or i - tgt < best[1] - best[0]):
            best = (tgt, i)
    return body[best[0]:best[1] + 1] if best else []


def main(argv):
    keep, inst, extra = None, POSE, []
    it = iter(argv)
    for a in it:
        if a == "--keep":
            keep = os.path.abspath(next(it))
        elif a == "--instance":
            inst = next(it)
        else:
            extra.append(a)
    lines = assemble(extra, keep)
    body, meta = function_body(lines, inst)
    fig = {}
    for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("sgprs", r"; TotalNumSgprs: (\d+)"), ("scratch_bytes", r"; ScratchSize: (\d+)"),
                     ("waves_per_simd", r"; Occupancy: (\d+)")):
        fig[key] = next(int(m.group(1)) for l in meta for m in [re.search(pat, l)] if m)
    first = next(i for i, l in enumerate(body) if op(l).startswith("global_load"))
    fig["lgkm_waits_before_first_global_load"] = sum(1 for l in body[:first] if op(l) == "s_waitcnt" and "lgkmcnt(0)" in l)
    fig["s_loads_before_first_global_load"] = sum(1 for l in body[:first] if op(l).startswith("s_load"))
    blk = [op(l) for l in step_block(body)]
    fig["step_block_v"] = sum(1 for o in blk if o.startswith("v_"))
    fig["step_block_ds"] = sum(1 for o in blk if o.startswith("ds_"))
    fig["step_block_s_cbranch"] = sum(1 for o in blk if o.startswith("s_cbranch"))
    fig["step_block_lines"] = sum(1 for o in blk if o)
    print(inst, " ".join(extra))
    for k, v in fig.items():
        print(f"  {k:40s} {v}")
    n, bad = scratch_of_every_instance(lines)
    print(f"  instances of both kernels: {n}, with scratch: {bad if bad else 'none'}")


if __name__ == "__main__":
    main(sys.argv[1:])
