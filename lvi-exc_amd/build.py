"""Build liblvx.so (HIP, gfx950 only) in-tree: python lvi-exc_amd/build.py [--force] [--verbose]."""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "liblvx.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fno-gpu-rdc", "-Wno-unused-result"] + os.environ.get("LVX_DEFINES", "").split()   # e.g. LVX_DEFINES=-DLVX_KTIME: cycle counters of the MFMA family kernel (debug print)
# FP contraction: the upstream kernels reproduce the reference's float arithmetic bit for bit (no FMA formation); the FP64
# residual / Jacobian / solver kernels are compared at 1e-12 relative and use FMAs.  The map rendering's projection rounds as the g++ build of its header does
# (tests/native/render_host_check.cpp): records are compared byte for byte.  The trajectory queries share lvx_pose.h with both: a sensor pose is the same bits in all three.
# The rotation initialisation's sums and 4 x 4 eigen-solver are held against the g++ build of lvx_rotinit.h (tests/native/rotinit_host_check.cpp).
# Every csrc/*.hip is named here: "off", or DEFAULT (fast unless LVX_CONTRACT overrides it).  A source that is not listed is an error, never a silent default.
DEFAULT = None
CONTRACT = {"lvx_upstream.hip": "off", "lvx_render.hip": "off", "lvx_traj.hip": "off", "lvx_rotinit.hip": "off",
            "lvx_handoff.hip": "off", "lvx_api.hip": DEFAULT, "lvx_bcr.hip": DEFAULT, "lvx_eval.hip": DEFAULT, "lvx_solver.hip": DEFAULT, "lvx_stats.hip": DEFAULT}
DEFAULT_CONTRACT = os.environ.get("LVX_CONTRACT", "fast")


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def contract(src):
    """-ffp-contract mode of one source (path or file name, with or without .hip)."""
    name = os.path.basename(src)
    name = name if name.endswith(".hip") else name + ".hip"
    if name not in CONTRACT:
        raise RuntimeError("%s has no entry in build.py's CONTRACT table: say 'off' or DEFAULT" % name)
    return CONTRACT[name] or DEFAULT_CONTRACT


def stale():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = sources() + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(HERE, "..", "include", "*.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not stale():
        return OUT
    objs = []
    procs = []
    modes = [(src, contract(src)) for src in sources()]   # (raises before anything is compiled)
    for src, mode in modes:
        obj = os.path.join(CSRC, os.path.basename(src)[:-4] + ".o")
        cmd = [HIPCC] + FLAGS + ["-ffp-contract=" + mode, "-c", src, "-o", obj]
        if verbose:
            cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
            print(" ".join(cmd), flush=True)
        procs.append((subprocess.Popen(cmd), cmd))
        objs.append(obj)
    for p, cmd in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs + ["-ldl", "-Wl,-rpath,/opt/rocm/lib"]   # rocBLAS / rocSOLVER are dlopen'ed on demand (bands wider than 208: lvx_bcr.hip), librccl likewise
    subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    if "--contract" in sys.argv:   # python build.py --contract FILE: the mode FILE is built with (tools/build_variant.sh)
        print(contract(sys.argv[sys.argv.index("--contract") + 1]))
        sys.exit(0)
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
