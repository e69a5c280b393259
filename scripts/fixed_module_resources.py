"""Register / scratch / LDS figures of the fixed-nonant lane module next to the
PH module's, per kernel: both sources (from the ABI emulation's test hooks,
the same generator the library feeds to hipRTC) compiled offline for gfx950
with -Rpass-analysis=kernel-resource-usage.  No GPU needed.

    python scripts/fixed_module_resources.py [farmer|aircond]
"""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sources(model):
    import mpisppy_amd  # noqa: F401
    from mpisppy_amd import _native, build
    import xhat_cases as xc
    build.build_emu(verbose=False)
    emu = _native.Lib(os.path.join(ROOT, "tests", "emu", "libphx_emu.so"), prefix="emu_phx_")
    ev, _ = xc.make_eval(emu, "cpu", *(("farmer", 200) if model == "farmer" else ("aircond", (4, 3, 2))))
    out = {}
    for name in ("lane_source", "fixed_lane_source"):
        fn = getattr(emu.lib, "emu_phx_" + name)
        fn.restype = ctypes.c_char_p
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out[name] = fn(ev._ctx, 2).decode()
    return out


def usage(src):
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "k.hip")
        open(f, "w").write(src)
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
                            "--cuda-device-only", "-I", os.path.join(ROOT, "mpi-sppy_amd", "csrc"),
                            "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "k.o"), f],
                           capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(r.stderr[-3000:])
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
        for key, pat in (("vgpr", r"VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None and key not in cur:
                cur[key] = int(m.group(1))
    return rows


def main():
    model = sys.argv[1] if len(sys.argv) > 1 else "farmer"
    src = sources(model)
    ph, fx = usage(src["lane_source"]), usage(src["fixed_lane_source"])
    print("%-22s %28s   %28s" % (model, "PH module", "fixed-nonant module"))
    print("%-22s %28s   %28s" % ("kernel", "VGPR AGPR scratch LDS occ", "VGPR AGPR scratch LDS occ"))
    for k in sorted(ph):
        a, b = ph[k], fx.get(k, {})
        fmt = lambda r: "%4s %4s %7s %5s %3s" % tuple(r.get(x, "-") for x in ("vgpr", "agpr", "scratch", "lds", "occ"))
        print("%-22s %28s   %28s" % (k, fmt(a), fmt(b)))


if __name__ == "__main__":
    main()
