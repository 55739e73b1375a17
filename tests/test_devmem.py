"""CPU: the owner of device memory (lz-ani_amd/csrc/lzani_devmem.h) under the allocation fault, in a stand-alone host
program under the address and undefined-behaviour sanitizers (tests/model/devmem_check.cpp: with every attempt refused
the HIP runtime is never called), and the C-ABI hook lzani_debug_alloc_fault through the binding."""
import os
import subprocess

import pytest

import lzani_ctypes as L
import util as U


def test_devmem_under_the_sanitizers(tmp_path):
    src = os.path.join(U.ROOT, "tests", "model", "devmem_check.cpp")
    exe = str(tmp_path / "devmem_check")
    subprocess.check_call(["hipcc", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(U.ROOT, "lz-ani_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[:2] == ["devmem_check", "ok"] and int(r.stdout.split()[2]) >= 40


def test_the_hook_through_the_binding():
    """No allocation is made here (there is no GPU): the call's own contract -- seen since the previous call, first = 0
    disarms, a range of no attempts is refused, the context manager disarms on every way out."""
    L.build_library()
    lib = L.load_library()
    L.alloc_fault(0)
    assert L.alloc_fault(0) == 0
    assert L.alloc_fault(5, L.ALLOC_FAULT_ALL) == 0 and L.alloc_fault(0) == 0
    assert lib.lzani_debug_alloc_fault(1, 1, None) == 0                     # seen may be NULL
    assert lib.lzani_debug_alloc_fault(1, 0, None) == -1                    # a range of nothing: LZANI_ERR_ARG, and ...
    with pytest.raises(L.LzaniError):
        with L.AllocFault(1, L.ALLOC_FAULT_ALL):
            raise L.LzaniError("inside")
    # ... whatever was armed, the way out of the block disarmed it: a context can be asked for (it fails for want of a
    # device or succeeds, but not with LZANI_ERR_NOMEM)
    f = L.AllocFault(1)
    with f:
        pass
    assert f.seen == 0
    import ctypes as C
    h = C.c_void_p()
    arr, _ = L.params_array(None)
    rc = lib.lzani_create(arr, 0, C.byref(h))
    assert rc in (0, -3), rc
    if rc == 0:
        lib.lzani_destroy(h)
