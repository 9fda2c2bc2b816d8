"""Build-time guard of the stream / stream-q conv kernels (no GPU needed): compiles tl_conv_stream.hip and tl_conv_streamq.hip for gfx950 to
assembly and checks, per kernel instantiation,

  1. registers: waves per SIMD not below, scratch bytes not above, the committed figures in tools/conv_epilogue_baseline.txt -- several
     instantiations sit one register step from losing a wave, and which epilogue form an instantiation takes (stream_epi_ahead /
     streamq_epi_ahead) was chosen by these figures;
  2. the epilogue rule for the kernels listed in FULL_AHEAD (the benchmark's: every residual block requested ahead): in the inference tail --
     from its first global store (after the `; tl_epi_lds_tail` marker) to the next s_endpgm -- there is no vector-memory load and no vmcnt wait.

    python tools/check_conv_epilogue.py            # check (exit status 1 on a violation)
    python tools/check_conv_epilogue.py --update   # rewrite the baseline from this build (after a deliberate change; review the diff)
"""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "treelearn_amd", "csrc")
BASE = os.path.join(ROOT, "tools", "conv_epilogue_baseline.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "--cuda-device-only", "-S"]
UNITS = ("tl_conv_streamq.hip", "tl_conv_stream.hip")
# demangled-name prefixes of the kernels that must keep the whole rule (template arguments as the demangler prints them)
FULL_AHEAD = (
    "k_conv_streamq<27, 2, 1, 2, 8, 1, 2, 1, false, false>",     # 64 -> 64   (level 2)
    "k_conv_streamq<27, 2, 2, 2, 8, 1, 2, 1, false, false>",     # 128 -> 64  (level 2 decoder)
    "k_conv_streamq<27, 3, 3, 2, 8, 1, 2, 1, false, false>",     # 192 -> 96  (level 3 decoder)
    "k_conv_streamq<27, 4, 2, 2, 8, 1, 2, 1, false, false>",     # 128 -> 128 (level 4)
    "k_conv_stream<true, 8, 2, 1, 3, 2, 2, false, false>",       # strided 32 -> 64, two row blocks per wave
)


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def compile_unit(unit, tmp):
    out = os.path.join(tmp, unit[:-4] + ".s")
    subprocess.run([HIPCC] + FLAGS + ["-c", os.path.join(CSRC, unit), "-o", out], check=True, capture_output=True)
    return open(out).read()


def kernels(asm):
    """-> {mangled name: (body lines, vgprs, scratch, occupancy)} from the per-kernel comment block hipcc writes after each function"""
    res = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.S | re.M):
        name, body = m.group(1), m.group(2)
        tail = asm[m.end():m.end() + 4000]
        g = lambda key: int(re.search(r";\s*%s:\s*(\d+)" % key, tail).group(1))
        res[name] = (body.split("\n"), g("NumVgprs"), g("ScratchSize"), g("Occupancy"))
    return res


def tail_violations(lines):
    """from the marker epi_wave_tail_lds leaves behind its wait (`; tl_epi_lds_tail`) to the next s_endpgm: nothing that loads from or waits for
    vector memory once the first store is out"""
    marks = [i for i, l in enumerate(lines) if "tl_epi_lds_tail" in l]
    if len(marks) != 1:
        return [f"{len(marks)} tail markers"]
    bad, started = [], False
    for l in lines[marks[0]:]:
        op = l.split("//")[0].split(";")[0].strip()
        if op.startswith("s_endpgm"):
            return bad if started else ["no store in the tail"]
        if op.startswith("global_store") or op.startswith("buffer_store"):
            started = True
        elif started and (re.match(r"(global_load|buffer_load|flat_load|scratch_load)", op) or (op.startswith("s_waitcnt") and "vmcnt" in op)):
            bad.append(op)
    return bad + ["no s_endpgm after the marker"]


def main():
    update = "--update" in sys.argv
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=2) as ex:
        asms = list(ex.map(lambda u: compile_unit(u, tmp), UNITS))
    ks = {}
    for a in asms:
        ks.update(kernels(a))
    names = demangle(sorted(ks))
    if update:
        with open(BASE, "w") as f:
            f.write("# waves per SIMD, scratch bytes per lane, VGPRs (information), kernel -- tools/check_conv_epilogue.py --update\n")
            for n in sorted(ks):
                f.write(f"{ks[n][3]} {ks[n][2]} {ks[n][1]} {n}\n")
        print(f"wrote {len(ks)} kernels to {BASE}")
        return 0
    base = {}
    for l in open(BASE):
        if l.strip() and not l.startswith("#"):
            occ, scr, _, n = l.split()
            base[n] = (int(occ), int(scr))
    bad = 0
    for n in sorted(ks):
        _, vg, scr, occ = ks[n]
        if n not in base:
            print(f"NEW (not in the baseline): {names[n]}: {vg} VGPRs, {scr} B scratch, {occ} waves per SIMD"); bad += 1
        elif occ < base[n][0] or scr > base[n][1]:
            print(f"WORSE: {names[n]}: waves per SIMD {base[n][0]} -> {occ}, scratch {base[n][1]} -> {scr} ({vg} VGPRs)"); bad += 1
    for n in sorted(set(base) - set(ks)):
        print(f"GONE: {n}"); bad += 1
    seen = set()
    for n in sorted(ks):
        for pre in FULL_AHEAD:
            if pre in names[n]:
                seen.add(pre)
                v = tail_violations(ks[n][0])
                if v:
                    print(f"RULE: {names[n]}: after the first store of the inference tail: {', '.join(v[:6])}"); bad += 1
    for pre in set(FULL_AHEAD) - seen:
        print(f"MISSING: no kernel matches {pre}"); bad += 1
    print(f"{len(ks)} kernels, {len(seen)} checked for the epilogue rule: " + ("OK" if not bad else f"{bad} violation(s)"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
