"""scripts/kernel_code_diff.py, the check behind byte-identical restructurings of the kernel sources: an object compared
with itself is identical, two objects that differ in one kernel are reported with that kernel's name.  The inputs are built
here from a few lines of HIP (no GPU: hipcc cross-compiles), never from the library -- a comparator that reads nothing, or
the wrong bytes, cannot pass."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = """
#include <hip/hip_runtime.h>
#ifndef SHIFT_OP
#define SHIFT_OP +
#endif
extern "C" __global__ void scale_kernel(float* x, float s, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= s;
}
extern "C" __global__ void shift_kernel(float* x, float s, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] SHIFT_OP s;
}
"""


@pytest.fixture(scope="module")
def kd():
    spec = importlib.util.spec_from_file_location("kernel_code_diff", os.path.join(ROOT, "scripts", "kernel_code_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def objects(kd, tmp_path_factory):
    """(plain, variant): the same two kernels, shift_kernel subtracting instead of adding in the second object."""
    d = tmp_path_factory.mktemp("kernel_code_diff")
    src = d / "two_kernels.hip"
    src.write_text(SOURCE)
    plain = kd.compile_device(str(src), str(d / "plain.co"))
    variant = kd.compile_device(str(src), str(d / "variant.co"), defines=["SHIFT_OP=-"])
    return plain, variant


def test_the_kernels_of_an_object_are_found(kd, objects):
    k = kd.read_kernels(objects[0])
    assert sorted(k) == ["scale_kernel", "shift_kernel"]
    for code, descriptor in k.values():
        assert len(code) > 0 and len(code) % 4 == 0 and len(descriptor) == 64 - 8


def test_an_object_is_identical_to_itself(kd, objects):
    r = kd.compare([objects[0]], [objects[0]])
    assert kd.identical(r) and (r["old"], r["new"]) == (2, 2)
    assert kd.report(r).splitlines() == ["kernels: 2 old, 2 new; 0 only old, 0 only new, 0 defined twice, 0 differ"]


def test_one_changed_kernel_is_reported_by_name(kd, objects):
    r = kd.compare([objects[0]], [objects[1]])
    assert not kd.identical(r)
    assert r["differ"] == ["shift_kernel"] and not r["only_old"] and not r["only_new"] and not r["twice"]
    assert kd.report(r).splitlines() == ["kernels: 2 old, 2 new; 0 only old, 0 only new, 0 defined twice, 1 differ",
                                         "  differ: shift_kernel"]


def test_a_kernel_in_two_units_of_one_side_is_reported(kd, objects):
    r = kd.compare([objects[0]], [objects[0], objects[0]])
    assert not kd.identical(r) and r["twice"] == ["scale_kernel", "shift_kernel"] and not r["differ"]
