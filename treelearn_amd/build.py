"""Build libtreelearn_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m treelearn_amd.build [--force]

The library is built IN-TREE (treelearn_amd/lib/) so it travels with the repo snapshot to the
GPU box; it is git-ignored.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libtreelearn_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


# units compiled a SECOND time with -DTL_F16_BUILD (csrc/tl_half.h): the same kernels with IEEE-half conversions and the f16 MFMA,
# launchers suffixed _f16 -- the float16 inference path (TL_F16)
F16_UNITS = ("tl_conv_direct.hip", "tl_conv_blk.hip", "tl_conv_up.hip", "tl_conv_stream.hip", "tl_conv_streamq.hip", "tl_conv_small.hip", "tl_conv_bf16.hip", "tl_head.hip",
             # the training units (csrc/tl_f16_train.h): weight gradients, BatchNorm train forward / backward, row gather / scatter-add, the heads' small Linears
             "tl_wgrad.hip", "tl_wgrad_dense.hip", "tl_wgrad_rows.hip", "tl_bn.hip", "tl_rows.hip", "tl_linear_small.hip")


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hdrs.append(os.path.join(os.path.dirname(HERE), "include", "treelearn_hip.h"))
    srcs = sources()
    objs = [os.path.join(objdir, os.path.basename(s)[:-4] + ".o") for s in srcs]
    jobs = [(s, o, []) for s, o in zip(srcs, objs)]
    for s in srcs:
        if os.path.basename(s) in F16_UNITS:
            o = os.path.join(objdir, os.path.basename(s)[:-4] + "_f16.o")
            objs.append(o); jobs.append((s, o, ["-DTL_F16_BUILD"]))

    def compile_one(so):
        s, o, extra = so
        if force or _stale(o, [s] + hdrs):
            cmd = [HIPCC] + FLAGS + extra + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
            return True
        return False

    with ThreadPoolExecutor(max_workers=6) as ex:
        changed = list(ex.map(compile_one, jobs))
    if force or any(changed) or _stale(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
