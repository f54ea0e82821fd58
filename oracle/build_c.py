"""Build the C restatement ``oracle/libbveval.so`` (test infrastructure / CPU
baseline only) and its wide twin ``oracle/libbveval_wide.so`` (``-DMAXW=64``: values
up to 4096 bits, 512-byte Keccak inputs; tests only, per-candidate cost grows with
MAXW).  Portable flags: the libraries travel to the GPU box host."""
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
SRC = HERE / "bveval.c"
LIB = HERE / "libbveval.so"
LIB_WIDE = HERE / "libbveval_wide.so"
WIDE_MAXW = 64  # 64-bit words per value in the wide library


def _build_one(lib: Path, defines, force: bool) -> Path:
    if not force and lib.exists() and lib.stat().st_mtime >= SRC.stat().st_mtime:
        return lib
    tmp = lib.with_suffix(".so.tmp")
    subprocess.run(["gcc", "-O3", "-std=c11", "-fopenmp", "-fPIC", "-shared", "-Wall", *defines, "-o", str(tmp),
                    str(SRC)], check=True)
    tmp.replace(lib)
    return lib


def build_wide(force: bool = False) -> Path:
    return _build_one(LIB_WIDE, [f"-DMAXW={WIDE_MAXW}"], force)


def build(force: bool = False) -> Path:
    build_wide(force)
    return _build_one(LIB, [], force)


if __name__ == "__main__":
    print(build(force=True))
