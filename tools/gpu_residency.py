"""How many light-tier workgroups does one CU of this device really hold?  (diagnostic; needs a GPU)

The light kernel is one 64-lane workgroup per env and LDS is what caps the envs per CU, but the hardware hands LDS out in blocks of a
size the compiler's occupancy remark knows nothing about.  This tool asks the device (tools/residency_probe.hip): one-wave workgroups
with N bytes of static LDS count themselves per CU while they wait a bounded time; the table is the largest count any CU reached.
It also prints what the runtime's occupancy calculator says for the product's light kernels.

   usage: python tools/gpu_residency.py [--sizes 12800,13312,...] [--wait-us 200] [--blocks-per-cu 16] [--lib build/residency_probe.so]
"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SRC = os.path.join(ROOT, "tools", "residency_probe.hip")
KEYS = 2048
LDS_PER_CU = 160 * 1024
LIGHT_KERNELS = ["_Z19jaco_physics_kernel12JacoStepArgs", "_Z26jaco_physics_kernel_listed12JacoStepArgs"]


def build(lib):
    if os.path.exists(lib) and os.path.getmtime(lib) > os.path.getmtime(SRC):
        return
    os.makedirs(os.path.dirname(os.path.abspath(lib)), exist_ok=True)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", lib])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12800,13312,13584,13824,14080")
    ap.add_argument("--wait-us", type=float, default=200.0)
    ap.add_argument("--blocks-per-cu", type=int, default=16, help="workgroups launched per CU (more than fit: the rest queue up behind)")
    ap.add_argument("--lib", default=os.path.join(ROOT, "build", "residency_probe.so"))
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    build(a.lib)
    if a.build_only:
        return
    sys.path.insert(0, ROOT)
    from mujoco_jaco_amd import _lib
    env = _lib.load()   # (torch's HIP runtime first, then the product library, then the probe: one runtime in the process)
    P = ctypes.CDLL(a.lib)
    P.residency_last_error.restype = ctypes.c_char_p
    P.residency_probe_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_float)]
    P.residency_occupancy.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]

    def check(rc):
        if rc != 0:
            raise RuntimeError("residency probe: %s" % P.residency_last_error().decode())

    cus, lds_cu, lds_blk = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(P.residency_device(ctypes.byref(cus), ctypes.byref(lds_cu), ctypes.byref(lds_blk)))
    print("device: %d CUs, LDS per CU %d B, per workgroup %d B (hipDeviceProp)" % (cus.value, lds_cu.value, lds_blk.value))
    for name in LIGHT_KERNELS:
        try:
            handle = ctypes.c_void_p.in_dll(env, name)
        except ValueError:
            print("hipOccupancyMaxActiveBlocksPerMultiprocessor(%s): symbol not exported" % name)
            continue
        n = ctypes.c_int()
        check(P.residency_occupancy(ctypes.addressof(handle), 64, 0, ctypes.byref(n)))
        print("hipOccupancyMaxActiveBlocksPerMultiprocessor(%s, 64 threads): %d workgroups per CU" % (name, n.value))
    print("probe: %d one-wave workgroups per CU launched, each waits %.0f us; peak = workgroups of one CU alive at once" % (a.blocks_per_cu, a.wait_us))
    print("%8s %8s %8s %8s %9s | fits by arithmetic: %6s %8s %9s" % ("LDS B", "CUs seen", "peak min", "peak max", "launch ms", "exact", "512-B", "1280-B"))
    peak = (ctypes.c_uint * KEYS)()
    ms = ctypes.c_float()
    for n in [int(x) for x in a.sizes.split(",")]:
        check(P.residency_probe_run(n, a.blocks_per_cu * cus.value, a.wait_us, peak, ctypes.byref(ms)))
        seen = [v for v in peak if v]
        fits = [LDS_PER_CU // (-(-n // g) * g) for g in (1, 512, 1280)]
        print("%8d %8d %8d %8d %9.3f | %25d %8d %9d" % (n, len(seen), min(seen), max(seen), ms.value, fits[0], fits[1], fits[2]))


if __name__ == "__main__":
    main()
