"""Compiles the reference itself (mhx/dwarfs) into oracle/_ref/libdwarfs_ref.so: its ricepp codec and its
nilsimsa, similarity and rsync hashes, unmodified, behind the C ABI of oracle/ref_driver.cpp.

    python oracle/ref_build.py [--force]

TEST INFRASTRUCTURE ONLY.  The reference tree is read at build time only (DWARFS_REFERENCE_ROOT, default
/root/reference); nothing of it and nothing compiled from it is committed -- oracle/_ref/ is ignored by git.
The one thing the reference needs that is not installed, range-v3, is stood in for by oracle/ref_shim/.

Flags: a release build (-DNDEBUG: the reference asserts clean low bits only in debug builds, and DwarFS ships
release builds), the portable `fallback` CPU variant and no RICEPP_CPU_BMI2* (the library may run on another
host than the one that built it), libstdc++ linked statically and kept out of the dynamic symbol table.
"""

from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path
from typing import Optional

HERE = Path(__file__).resolve().parent
OUT_DIR = HERE / "_ref"
LIB_PATH = OUT_DIR / "libdwarfs_ref.so"
OWN_SOURCES = [HERE / "ref_driver.cpp", Path(__file__).resolve(), *sorted((HERE / "ref_shim").rglob("*.hpp"))]
REFERENCE_SOURCES = ["ricepp/ricepp.cpp", "ricepp/ricepp_cpuspecific.cpp", "ricepp/cpu_variant.cpp",
                     "src/writer/internal/nilsimsa.cpp", "src/writer/internal/similarity.cpp"]
REFERENCE_INCLUDES = ["ricepp/include", "ricepp", "include"]
# the reference's headers that these sources and the driver include: a change to one rebuilds the library too
REFERENCE_HEADERS = ["ricepp/*.h", "ricepp/include/ricepp/**/*.h", "include/dwarfs/compiler.h",
                     "include/dwarfs/writer/internal/cyclic_hash.h", "include/dwarfs/writer/internal/nilsimsa.h",
                     "include/dwarfs/writer/internal/similarity.h"]
FLAGS = ["-std=c++20", "-O2", "-DNDEBUG", "-march=x86-64-v2", "-fPIC", "-static-libstdc++", "-static-libgcc",
         "-DRICEPP_CPU_VARIANT=fallback"]
LINK_FLAGS = ["-shared", "-Wl,--exclude-libs,ALL"]


def reference_root() -> Optional[Path]:
    """The reference tree, or None when it is not on this machine."""
    root = Path(os.environ.get("DWARFS_REFERENCE_ROOT", "/root/reference"))
    return root if all((root / s).is_file() for s in REFERENCE_SOURCES) else None


def flags_string() -> str:
    return " ".join(FLAGS)


def build(force: bool = False) -> Optional[Path]:
    """Builds the library if the reference tree is present and the library is missing or older than a source.
    Without the tree, leaves oracle/_ref/ as it is; returns the library's path if there is one, else None."""
    root = reference_root()
    if root is None:
        return LIB_PATH if LIB_PATH.exists() else None
    sources = [root / s for s in REFERENCE_SOURCES]
    headers = [h for pattern in REFERENCE_HEADERS for h in sorted(root.glob(pattern))]
    if not force and LIB_PATH.exists() and all(LIB_PATH.stat().st_mtime >= s.stat().st_mtime
                                               for s in OWN_SOURCES + sources + headers):
        return LIB_PATH
    OUT_DIR.mkdir(parents=True, exist_ok=True)
    tmp = LIB_PATH.with_suffix(f".so.tmp{os.getpid()}")
    cmd = [os.environ.get("CXX", "g++"), *FLAGS, f'-DREF_BUILD_FLAGS="{flags_string()}"', *LINK_FLAGS,
           "-I", str(HERE / "ref_shim"), *[a for i in REFERENCE_INCLUDES for a in ("-I", str(root / i))],
           "-o", str(tmp), str(HERE / "ref_driver.cpp"), *map(str, sources)]
    try:
        subprocess.run(cmd, check=True)
        tmp.replace(LIB_PATH)  # (atomic: a concurrent loader sees the old or the new library)
    finally:
        tmp.unlink(missing_ok=True)
    return LIB_PATH


if __name__ == "__main__":
    path = build(force="--force" in sys.argv[1:])
    print(path if path else "reference tree not found: nothing built")
