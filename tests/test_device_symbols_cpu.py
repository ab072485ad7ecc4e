"""CPU check that every kernel the host half of libsatt_hip.so registers exists in its device code, and the other way round.

hipcc compiles a .hip file twice.  The host half gets, per kernel, a launch stub (a FUNC whose mangled name carries
`__device_stub__<kernel>`) and an 8-byte handle OBJECT under the kernel's own mangled name, which the HIP runtime resolves by NAME
against the gfx950 code object at the first launch.  The device half defines `<mangled kernel>` and its kernel descriptor
`<mangled kernel>.kd`.  An object whose two halves do not come from the same source text still links and loads; the first launch of
the orphaned kernel then aborts the process on the GPU.  Both halves are plain ELF symbol tables, so the mismatch is visible here
with llvm-objdump / llvm-readelf, before anything is launched.  No list of kernels: both directions are derived from the library."""
import os
import re
import shutil
import subprocess

import pytest

import satt_amd  # noqa: F401

LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
STUB = "__device_stub__"


def symbols(path):
    """(type, size, section index, mangled name, demangled name) of every entry of the ELF's symbol tables: llvm-readelf lists them
    twice in the same order, as they are and with --demangle (an extern "C" name comes back as it is)"""
    def table(*flags):
        out = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "-sW", *flags, path], check=True, capture_output=True, text=True).stdout
        rows = [line.split(None, 7) for line in out.splitlines()]
        return [f for f in rows if len(f) == 8 and f[0].endswith(":") and f[0][:-1].isdigit()]
    plain, pretty = table(), table("--demangle")
    assert len(plain) == len(pretty) and all(a[:7] == b[:7] for a, b in zip(plain, pretty))
    return [(a[3], int(a[2]), a[6], a[7].strip(), b[7].strip()) for a, b in zip(plain, pretty)]


def kernel_of_stub(demangled_stub):
    """the kernel's demangled name from its launch stub's: the stub is the kernel's host twin under `__device_stub__<name>`, same
    scope, same template arguments, same parameters"""
    assert demangled_stub.count(STUB) == 1, demangled_stub
    return demangled_stub.replace(STUB, "")


@pytest.fixture(scope="module")
def halves(tmp_path_factory):
    import __graft_entry__ as ge
    so = ge.build()
    tmp = tmp_path_factory.mktemp("device_symbols")
    lib = os.path.join(str(tmp), "lib.so")
    shutil.copyfile(so, lib)
    subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=str(tmp))
    objs = sorted(os.path.join(str(tmp), f) for f in os.listdir(str(tmp)) if f.startswith("lib.so.") and f.endswith("gfx950"))
    assert objs, "no gfx950 code object in " + so
    host = symbols(lib)
    # demangled kernel name -> mangled stub name; the 8-byte handles by their mangled names, which is what the runtime looks up
    stubs = {kernel_of_stub(d): n for t, _, ndx, n, d in host if t == "FUNC" and ndx != "UND" and STUB in n}
    handles = {n for t, size, ndx, n, _ in host if t == "OBJECT" and size == 8 and ndx != "UND"}
    kds = {}          # mangled kernel name -> demangled
    for o in objs:
        dev = symbols(o)
        defined = {n: d for t, _, ndx, n, d in dev if t == "FUNC" and ndx != "UND"}
        for t, _, ndx, n, _ in dev:
            if t == "OBJECT" and ndx != "UND" and n.endswith(".kd"):
                assert n[:-3] in defined, "descriptor without its kernel in the same code object: " + n
                kds[n[:-3]] = defined[n[:-3]]
    return stubs, handles, set(kds), kds


def test_kernel_of_stub():
    assert kernel_of_stub("(anonymous namespace)::__device_stub__adam_k(float*, float const*)") == "(anonymous namespace)::adam_k(float*, float const*)"
    assert kernel_of_stub("void __device_stub__foo<3>(float*)") == "void foo<3>(float*)"
    assert kernel_of_stub("__device_stub__plain_c_kernel") == "plain_c_kernel"


def test_every_registered_kernel_has_device_code(halves):
    stubs, handles, kds, names = halves
    assert len(stubs) > 100 and len(kds) > 100          # (the library holds several hundred instantiations)
    device = {names[k]: k for k in kds}
    missing = sorted(k for k in stubs if k not in device)
    assert not missing, "host stubs whose kernel has no .kd in any gfx950 code object: %s" % missing[:5]
    unhandled = sorted(k for k in stubs if device[k] not in handles)
    assert not unhandled, "host stubs without the 8-byte kernel handle the runtime looks the device symbol up by: %s" % unhandled[:5]


def test_every_device_kernel_has_a_host_handle(halves):
    stubs, handles, kds, names = halves
    orphans = sorted(k for k in kds if k not in handles)
    assert not orphans, "device kernels the host half does not register: %s" % orphans[:5]
    unlaunched = sorted(names[k] for k in kds if names[k] not in stubs)
    assert not unlaunched, "device kernels without a host launch stub: %s" % unlaunched[:5]


@pytest.mark.parametrize("kernel", ["dec_stop_scan_k", "dec_ends_scan_k"])
def test_scan_kernels_on_both_sides(halves, kernel):
    stubs, handles, kds, names = halves
    host = [k for k in stubs if re.search(r"\b%s\(" % kernel, k)]
    assert len(host) == 1, host
    dev = [k for k in kds if names[k] == host[0]]
    assert len(dev) == 1 and dev[0] in handles, dev
