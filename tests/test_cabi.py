"""CPU tier: the C-ABI library loads, exports every symbol include/ludvm_hip.h declares, and the
ctypes table binds exactly that set.  No compute calls (there is no GPU in this tier)."""
import os
import re

import pytest

from conftest import ROOT
from ludvm_amd import _ffi


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ludvm_[a-z0-9_]+)\s*\(", text))


def test_library_is_built_in_tree():
    assert os.path.exists(_ffi.LIB_PATH), "run __graft_entry__.build() (make -C ludvm_amd/csrc)"
    assert os.path.dirname(_ffi.LIB_PATH).endswith(os.path.join("ludvm_amd", "csrc"))


def test_header_library_and_binding_agree():
    declared = _declared_symbols()
    assert len(declared) >= 27
    assert declared == set(_ffi.SIGNATURES), declared ^ set(_ffi.SIGNATURES)
    lib = _ffi.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in ludvm_hip.h but not exported"
    assert lib.ludvm_abi_version() == _ffi.ABI_VERSION


def test_production_library_reads_no_experiment_switch():
    """a production build's bits must not depend on the environment.  The A/B switches of rounds 1-3
    and the negative codes of ludvm_set_sym_tuning live behind -DLUDVM_EXPERIMENTS (libludvm_hip_exp.so); the product's
    object file does not even contain their names, and the only variables it reads cannot change a result."""
    import re
    moved = ("LUDVM_SYM_MIXED", "LUDVM_SYM_TAIL_ITEMS", "LUDVM_SYM_QUAD", "LUDVM_SYM_QUAD_MIN_TILES", "LUDVM_SMALL_TILE_MAX",
             "LUDVM_SMALL_TILE_MAX_F64", "LUDVM_MARCH_OVERLAP", "LUDVM_MARCH_EXT_EVENTS", "LUDVM_GRID_KERNEL", "LUDVM_FEW_PACKED",
             "LUDVM_XCD_RUN", "LUDVM_ALLOW_ANY_ARCH")

    def names(path):
        return set(m.decode() for m in re.findall(rb"LUDVM_[A-Z0-9_]+", open(path, "rb").read()))
    prod, exp = names(_ffi.LIB_PATH), names(_ffi.EXP_LIB_PATH)
    assert not (prod & set(moved)), prod & set(moved)
    assert {"LUDVM_RCCL_LIB", "LUDVM_COMM_FORCE"} <= prod
    assert set(moved) - {"LUDVM_ALLOW_ANY_ARCH"} <= exp          # ... and the measurement build has them all
    # both builds export the same ABI
    exp_lib = _ffi.load(_ffi.EXP_LIB_PATH)
    assert exp_lib.ludvm_abi_version() == _ffi.ABI_VERSION
    # the source reads the environment through the one macro (plus the two production variables)
    import glob
    csrc = os.path.join(ROOT, "ludvm_amd", "csrc")
    units = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    assert len(units) == 9          # context, launch, comm, order, induce, wake, march, flowfield + spatial_order (ctx.hpp)
    direct = [v for u in units for v in re.findall(r'std::getenv\("(\w+)"\)', open(u).read())]
    assert sorted(direct) == ["LUDVM_COMM_FORCE", "LUDVM_RCCL_LIB"], direct
    # the measurement build recompiles only the units that read a switch (EXP_UNITS): a switch in any other unit would do nothing
    readers = {os.path.basename(u)[:-4] for u in units if re.search(r"LUDVM_EXP_ENV|LUDVM_EXPERIMENTS", open(u).read())}
    exp_units = re.search(r"^EXP_UNITS\s*=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert readers == set(exp_units), (readers, exp_units)
    for hdr in glob.glob(os.path.join(csrc, "*.hpp")):
        text = open(hdr).read()
        assert "getenv" not in text.replace("#define LUDVM_EXP_ENV(name) std::getenv(name)", ""), hdr


def test_every_entry_point_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "ludvm_hip.h")).read()
    assert text.count("LUDVM.py:") >= 15


def test_no_cpu_fallback_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ludvm_amd import Engine, LUDVM, LudvmHipError
    with pytest.raises(LudvmHipError):
        Engine(0)
    with pytest.raises(LudvmHipError):
        LUDVM(tf=0.1, verbose=False)   # the product constructor needs the HIP engine


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(OSError):
        _ffi.load(str(tmp_path / "libludvm_hip.so"))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "ludvm_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("the oracle", "").replace("oracle to cover", "") or f == "sharded.py", f
                assert "import oracle" not in src and "from oracle" not in src, f


def test_tools_and_bench_do_not_use_the_oracle_outside_the_cpu_baseline():
    """Only tests/ (incl. tests/tools/), __graft_entry__.smoke() and bench.py's cpu_baseline leg may import the oracle."""
    import re
    for f in sorted(os.listdir(os.path.join(ROOT, "tools"))):
        if f.endswith(".py") or f.endswith(".sh"):
            src = open(os.path.join(ROOT, "tools", f)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f
    bench = open(os.path.join(ROOT, "bench.py")).read()
    hits = [m.start() for m in re.finditer(r"from oracle|import oracle", bench)]
    a, b = bench.index("def cpu_baseline("), bench.index("def main(")
    assert hits and all(a < h < b for h in hits)


def test_single_hip_runtime_whatever_the_import_order():
    """PyTorch-ROCm bundles its own libamdhip64.so; the engine must share it rather than map the system
    copy next to it (two runtimes in one process: torch cannot initialise its device afterwards, stream
    handles cross runtimes).  Load the engine first, torch second, and count the mapped runtimes."""
    import subprocess
    import sys
    code = (
        "from ludvm_amd import _ffi\n"
        "_ffi.load()\n"
        "import torch\n"
        "libs = {l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l or 'libhsa-runtime64' in l}\n"
        "print(len(libs))\n"
        "print(sorted(libs))\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines()[0] == "2", out.stdout      # one HIP runtime + one HSA runtime


def test_every_entry_point_rejects_a_null_context():
    """No entry point may dereference a NULL context: all of them return LUDVM_E_ARG (none needs a GPU for that)."""
    import ctypes
    lib = _ffi.load()
    skipped = {"ludvm_abi_version", "ludvm_create", "ludvm_last_error"}
    for name, argtypes in _ffi.SIGNATURES.items():
        if name in skipped:
            continue
        args = []
        for t in argtypes[1:]:
            if t in (ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t):
                args.append(0)
            elif t in (ctypes.c_double, ctypes.c_float):
                args.append(0.0)
            else:
                args.append(None)      # every pointer type, c_void_p and c_char_p included
        rc = getattr(lib, name)(None, *args)
        assert rc == _ffi.E_ARG, (name, rc)
    assert lib.ludvm_last_error(None) == b"null context"
    assert lib.ludvm_create(0, None) != _ffi.OK          # null output pointer


def test_inline_asm_keeps_clear_of_the_transcendental_hazard(tmp_path):
    """The symmetric kernel's packed-target multiply is inline assembly (v_pk_mul_f32 with op_sel) that reads the result
    of v_rsq_f32.  gfx950 needs one issue slot between a transcendental instruction and a VALU read of its result, and
    the compiler's hazard pass does not look inside inline assembly (pair_sym_kernels.hpp, pk_mul_sel): check the ISA."""
    import re
    import subprocess
    src = os.path.join(ROOT, "ludvm_amd", "csrc", "launch.hip")          # (the unit that instantiates every pair kernel)
    out = tmp_path / "ludvm.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                    "--cuda-device-only", "-S", "-o", str(out), src], check=True, capture_output=True)
    code = [l.strip() for l in open(out) if l.strip() and not l.strip().startswith((";", "."))]
    asm_muls = 0
    for i, l in enumerate(code):
        if not (l.startswith(("v_pk_mul_f32", "v_pk_add_f32")) and "op_sel" in l):
            continue
        asm_muls += l.startswith("v_pk_mul_f32")
        read = set()
        for m in re.finditer(r"v\[(\d+):(\d+)\]", l.split(",", 1)[1]):
            read.update(range(int(m.group(1)), int(m.group(2)) + 1))
        prev = re.match(r"v_(rsq|rcp|sqrt|exp|log|sin|cos)_f\d+\w* v(\d+),", code[i - 1])
        assert not (prev and int(prev.group(2)) in read), (code[i - 1], l)
    assert asm_muls >= 100          # the check looked at the kernels it is meant for


def test_hot_kernels_do_not_spill():
    """Register budget of the pair kernels as hipcc compiles them for gfx950 (no GPU needed): no scratch, and the
    512-vortex symmetric tile within three waves per SIMD.  (A reduction buffer in LDS once pushed that kernel to ~300
    registers with spills inside its rotation loop: profiles/r02_packed_targets_ab.txt.)"""
    import re
    import subprocess
    src = os.path.join(ROOT, "ludvm_amd", "csrc", "launch.hip")          # (the unit that instantiates every pair kernel)
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.devnull],
                         check=True, capture_output=True, text=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            kernels[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1)
            kernels[cur][k.strip()] = v.strip()
    pair = {k: v for k, v in kernels.items() if "pair_f32" in k or "pair_sym_f32" in k or "pair_f64" in k}
    assert len(pair) >= 30, sorted(kernels)
    for name, r in pair.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["AGPRs"]) == 0, (name, r)
    t8 = {k: v for k, v in pair.items() if "pair_sym_f32ILi8" in k}
    assert len(t8) == 4        # mixed granularity (default), and 1, 2, 4 waves per work item
    for name, r in t8.items():
        assert int(r["VGPRs"]) <= 168 and int(r["Occupancy [waves/SIMD]"]) >= 3, (name, r)


def test_library_exports_the_c_abi_and_nothing_else():
    """The library is several translation units (ctx.hpp lists them) built with -fvisibility=hidden and linked under the
    version script csrc/exports.map: the dynamic symbol table holds the entry points include/ludvm_hip.h declares and NOTHING
    else -- no function the units offer each other (launch_pair, wake_grow, reduce_accumulators ...), no weak instantiation of
    the standard library, no destructor, no kernel handle (round 6: rounds 4-5 excused weak symbols and data objects)."""
    import subprocess
    for lib in (_ffi.LIB_PATH, _ffi.EXP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        defined = {l.split()[2] for l in out.splitlines() if len(l.split()) == 3}
        assert defined == _declared_symbols(), sorted(defined ^ _declared_symbols())[:10]


def test_every_non_template_kernel_header_belongs_to_one_unit():
    """A non-template __global__ function defined in a header that two units include would be defined twice.  Templates and
    device helpers live in pair_kernels.hpp / pair_sym_kernels.hpp / sym_rule.hpp (includable anywhere, no plain kernel inside); each of the
    other kernel headers is included by exactly one .hip file."""
    import glob
    csrc = os.path.join(ROOT, "ludvm_amd", "csrc")
    units = {os.path.basename(u): open(u).read() for u in glob.glob(os.path.join(csrc, "*.hip"))}
    owners = {"sym_prepare_kernels.hpp": "launch.hip", "induce_kernels.hpp": "induce.hip", "wake_kernels.hpp": "wake.hip",
              "march_kernels.hpp": "march.hip", "field_kernels.hpp": "flowfield.hip", "order_kernels.hpp": "order.hip"}
    for hdr, owner in owners.items():
        users = sorted(u for u, text in units.items() if f'#include "{hdr}"' in text)
        assert users == [owner], (hdr, users)
        assert f'#include "{hdr}"' not in open(os.path.join(csrc, "ctx.hpp")).read()
    for shared in ("pair_kernels.hpp", "pair_sym_kernels.hpp", "sym_rule.hpp", "march_types.hpp"):
        text = open(os.path.join(csrc, shared)).read()
        # every kernel in a shared header is a template (its __global__ line is preceded by a template line)
        lines = text.splitlines()
        for i, l in enumerate(lines):
            if l.startswith("__global__"):
                assert lines[i - 1].startswith("template"), (shared, i + 1, l)
