"""The Python side's one calling convention (v2v_amd/_lib.py: ptr, launch, DTYPE_CODES): what ptr gives for CPU tensors, that no other
module of the package brings a copy of its own, and that the dtype map holds exactly the codes of include/v2v_hip.h.  No GPU."""
import ctypes
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = sorted(p for p in glob.glob(os.path.join(ROOT, "v2v_amd", "*.py")) if os.path.basename(p) != "_lib.py")


@pytest.fixture(scope="module")
def L():
    from v2v_amd import _lib
    return _lib


def test_ptr_of_none_is_null(L):
    assert L.ptr(None) is None and L.ptr(None, 3) is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ptr_is_the_address_and_the_offset_counts_elements(L, dtype):
    t = torch.zeros(8, dtype=dtype)
    assert L.ptr(t).value == t.data_ptr()
    assert L.ptr(t, offset_elems=3).value == t.data_ptr() + 3 * t.element_size()
    assert L.ptr(t, 3).value == L.ptr(t[3:]).value


def test_ptr_keeps_the_address_of_an_empty_view(L):
    """The helper does not guess: it passes on the address the tensor reports and never looks at numel(); NULL for "no elements" is the call
    site's to say.  Current torch reports address 0 for every tensor without elements, a view of a non-empty tensor included, so the real
    view below only shows that ptr hands on what data_ptr() says (as a pointer, not as None).  The assertion that numel() is not consulted
    is carried by the stand-in: no elements, a non-zero address, and the address comes out."""
    t = torch.zeros(8, dtype=torch.float32)
    view = t[2:2]
    assert view.numel() == 0
    p = L.ptr(view)
    assert isinstance(p, ctypes.c_void_p) and (p.value or 0) == view.data_ptr()

    class NoElements:
        def numel(self):
            return 0

        def element_size(self):
            return 4

        def data_ptr(self):
            return 0x1000

    assert L.ptr(NoElements()).value == 0x1000 and L.ptr(NoElements(), 2).value == 0x1008


def test_the_modules_are_all_there():
    assert len(MODULES) >= 20 and {"nhwc_ops.py", "loss_ops.py", "esim.py", "metrics.py", "nernet.py"} <= {os.path.basename(p) for p in MODULES}


@pytest.mark.parametrize("path", MODULES, ids=[os.path.basename(p) for p in MODULES])
def test_no_module_brings_its_own_calling_convention(path):
    src = open(path).read()
    for needle in ("c_void_p(", "stream_ptr("):
        assert needle not in src, f"{os.path.basename(path)} spells out {needle}...): pointers and the stream come from _lib.ptr / _lib.launch"
    own = re.findall(r"^\s*def\s+(_ptr|_p|_launch|_lp_launch)\s*\(", src, flags=re.M)
    assert not own, f"{os.path.basename(path)} defines {own}: use _lib.ptr / _lib.launch"


def test_the_dtype_map_holds_the_codes_of_the_header(L):
    header = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    enum = re.search(r"typedef enum v2v_dtype \{(.*?)\} v2v_dtype;", header, flags=re.S).group(1)
    codes = {name: int(value) for name, value in re.findall(r"V2V_(\w+)\s*=\s*(\d+)", enum)}
    assert codes == {"U8": 0, "F32": 1, "F64": 2, "BF16": 3}
    assert L.DTYPE_CODES == {torch.uint8: codes["U8"], torch.float32: codes["F32"], torch.float64: codes["F64"], torch.bfloat16: codes["BF16"]}
    assert (L.U8, L.F32, L.F64, L.BF16) == (codes["U8"], codes["F32"], codes["F64"], codes["BF16"])
