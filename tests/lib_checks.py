"""What the host-side tests of the six C-ABI libraries share: reading a shipped library's dynamic symbols and its gfx950 code
object, reading product sources, and building a library's sources for the host against the SIMT emulator.  A plain module
(not a conftest): the tests import it and keep their own assertions.  Test infrastructure only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
COMMON_CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_common")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_COMMON_DIR = os.path.join(ROOT, "tests", "emu_common")      # the emulator twin of csrc_common/ccnet_device.hpp
HOST_CXX = "/opt/rocm/lib/llvm/bin/clang++"
LLVM_BIN = "/opt/rocm/lib/llvm/bin"
HAVE_LLVM_BINUTILS = os.path.exists(f"{LLVM_BIN}/clang-offload-bundler")
SPILL_FIELDS = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def exported_symbols(lib_path):
    """Sorted names of every defined dynamic symbol of the library (``nm -D --defined-only``)."""
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def code_object_kernels(lib_path, tmp_path, prefix):
    """{mangled kernel name: metadata dict} of the kernels whose name starts with ``prefix`` (the mangled namespace, such as
    "_ZN4ohem"), read from the notes of the gfx950 code object inside the shipped library."""
    fat, co = str(tmp_path / "lib.fatbin"), str(tmp_path / "lib.co")
    subprocess.run([f"{LLVM_BIN}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib_path, fat], check=True)
    subprocess.run([f"{LLVM_BIN}/clang-offload-bundler", "--unbundle", "--type=o",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM_BIN}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    kernels, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key == "name":               # a kernel's, or one of its arguments': the resource fields follow the kernel's
            cur = kernels.setdefault(val, {}) if val.startswith(prefix) else None
        elif cur is not None and key in SPILL_FIELDS + ("vgpr_count",):
            cur[key] = int(val)
    return kernels


def kernels_using_scratch(kernels, fields=SPILL_FIELDS):
    """The kernels of ``code_object_kernels`` with a nonzero ``fields`` entry: scratch memory or spilled registers."""
    return {n: k for n, k in kernels.items() if any(k.get(f, 0) for f in fields)}


def product_sources(*dirs):
    """{file name: text} of every .hip / .hpp under the given source directories."""
    return {f: open(os.path.join(d, f)).read() for d in dirs for f in sorted(os.listdir(d)) if f.endswith((".hip", ".hpp"))}


def build_emu_library(out, unit, include_dirs, reads=(), force=False):
    """Compile ``unit`` (an x_api.hip, or a .cpp that includes one) for the host, with tests/emu/hip_emu.cpp, into the shared
    library ``out``.  ``include_dirs`` go on the include path in the order given, the emulator's directories FIRST, so that
    <x_platform.hpp> resolves to the emulator twin.  Rebuilt when any source in those directories, or in ``reads`` (directories
    whose headers are included by relative path), is newer than ``out``."""
    runtime = os.path.join(EMU_DIR, "hip_emu.cpp")
    srcs = [unit, runtime] + [os.path.join(d, f) for d in list(include_dirs) + list(reads) for f in os.listdir(d)
                              if f.endswith((".hip", ".hpp", ".cpp", ".h"))]
    if not force and os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(s) for s in srcs):
        return out
    cxx = HOST_CXX if os.path.exists(HOST_CXX) else "g++"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-pass-failed"]
                   + ["-I" + d for d in include_dirs] + [unit, runtime, "-o", out], check=True, cwd=ROOT)
    return out


def build_shared_scaffold_emu(name, force=False):
    """The emulator build of ccnet_amd/csrc_<name>/<name>_api.hip for the four libraries on the shared scaffold
    (ohem, eval, lovasz, abn) -> tests/emu_<name>/lib<name>_emu.so."""
    csrc, emu = os.path.join(ROOT, "ccnet_amd", "csrc_" + name), os.path.join(ROOT, "tests", "emu_" + name)
    return build_emu_library(os.path.join(emu, f"lib{name}_emu.so"), os.path.join(csrc, name + "_api.hip"),
                             [emu, EMU_DIR, csrc, INCLUDE], reads=(EMU_COMMON_DIR, COMMON_CSRC), force=force)
