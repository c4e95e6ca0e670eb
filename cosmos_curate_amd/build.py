"""Build libcchot.so (the C-ABI hot-path library) with hipcc for gfx950.

Built IN-TREE (cosmos_curate_amd/lib/libcchot.so) so the .so travels with
the gpurun snapshot; .gitignore keeps it out of history.  Idempotent: object
files rebuild only when sources are newer.

Per-file flags:
- cc_pixel.hip: -ffp-contract=off — the pixel kernels promise bit-exact f32
  arithmetic vs the numpy oracle (oracle/color.py); FMA contraction would
  change rounding.
- cc_gemm.hip: default contraction (MFMA does the math anyway), packed-f32
  instructions off: the 256² epilogue works on adjacent register pairs, which
  hipcc would otherwise turn into v_pk_mul_f32 / v_pk_fma_f32 by the thousand.
- cc_motion.hip: integer arithmetic only; no floating-point flags matter.
- cc_conv.hip: default contraction (MFMA, and an FMA first layer whose
  tolerance is the f32 accumulation bound, not bit-exactness).
- cc_tnheads.hip: -ffp-contract=off — the histogram head is bit-equal to its
  numpy restatement, and the f32 chains say fmaf where they mean it.
- cc_attnpool.hip: default contraction (MFMA; f32 softmax within a stated
  bound), packed-f32 instructions off.
- cc_attncross.hip: cc_attnpool.hip's flags, for the same reasons.
- cc_kmeans.hip: cc_dedup.hip's flags plus packed-f32 instructions off, as for
  cc_attnpool.hip; the arithmetic is the f32 MFMA and ordered f64 adds, so
  contraction has nothing to contract.
- cc_dedupseg.hip: cc_kmeans.hip's flags, for the same f32 MFMA and compares.
- cc_motionscore.hip: -ffp-contract=off — the magnitude and the bilinear blend
  are the f32 chains of the torch path and of oracle/motion.py, product by
  product; an FMA would round them differently.
"""

from __future__ import annotations

import pathlib
import subprocess

PKG = pathlib.Path(__file__).resolve().parent
CSRC = PKG / "csrc"
LIBDIR = PKG / "lib"
LIB = LIBDIR / "libcchot.so"

HIPCC = "hipcc"
ARCH = "--offload-arch=gfx950"
COMMON = ["-O3", "-std=c++17", "-fPIC", f"-I{PKG.parent}"]
# no packed-f32 instructions (v_pk_mul_f32 and kin): the f32 rescale and
# softmax chains compile to the scalar forms
NO_PK_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]

SOURCES: list[tuple[str, list[str]]] = [
    ("cc_demux.cpp", []),
    ("cc_decode.cpp", []),
    ("cc_pixel.hip", [ARCH, "-ffp-contract=off"]),
    ("cc_gemm.hip", [ARCH, *NO_PK_F32]),
    ("cc_dedup.hip", [ARCH]),
    ("cc_ln.hip", [ARCH]),
    ("cc_attn.hip", [ARCH]),
    ("cc_motion.hip", [ARCH]),
    ("cc_conv.hip", [ARCH]),
    ("cc_tnheads.hip", [ARCH, "-ffp-contract=off"]),
    ("cc_attnpool.hip", [ARCH, *NO_PK_F32]),
    ("cc_attncross.hip", [ARCH, *NO_PK_F32]),
    ("cc_kmeans.hip", [ARCH, *NO_PK_F32]),
    ("cc_dedupseg.hip", [ARCH, *NO_PK_F32]),
    ("cc_motionscore.hip", [ARCH, "-ffp-contract=off"]),
]


def _needs_build(src: pathlib.Path, obj: pathlib.Path) -> bool:
    if not obj.exists():
        return True
    dep = [src, *CSRC.glob("*.hpp"), PKG.parent / "include" / "cc_hotpath.h"]
    return any(d.stat().st_mtime > obj.stat().st_mtime for d in dep)


def build(verbose: bool = True) -> pathlib.Path:
    LIBDIR.mkdir(exist_ok=True)
    objs = []
    rebuilt = False
    for name, extra in SOURCES:
        src = CSRC / name
        obj = LIBDIR / (src.stem + ".o")
        objs.append(obj)
        if _needs_build(src, obj):
            cmd = [HIPCC, *COMMON, *extra, "-c", str(src), "-o", str(obj)]
            if verbose:
                print("[cc build]", " ".join(cmd))
            subprocess.run(cmd, check=True)
            rebuilt = True
    if rebuilt or not LIB.exists():
        cmd = [HIPCC, ARCH, "-shared", "-fPIC", *map(str, objs), "-o", str(LIB)]
        if verbose:
            print("[cc build]", " ".join(cmd))
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    build()
