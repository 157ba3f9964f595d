"""The in-tree native libraries resolve every symbol at load time (dlopen RTLD_NOW) on the CPU, so a
kernel-library link error -- a host function declared in kernels.h and referenced by bindings.cpp
but never defined -- fails the CPU tier instead of the first GPU run; and the op schema the Python
layer calls exists in both the bf16 and the IEEE-fp16 build."""
import ctypes
import os

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "azure_hc_intel_tf_amd")
LIBS = ["_hcb_kernels.so", "_hcb_kernels_f16.so", "_hcb_comm.so"]


@pytest.mark.parametrize("name", LIBS)
def test_native_library_resolves_all_symbols(name):
    import torch  # noqa: F401  (the libraries link against libtorch / libc10, loaded by torch)

    path = os.path.join(PKG, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not built (python __graft_entry__.py builds it)")
    ctypes.CDLL(path, mode=os.RTLD_NOW | os.RTLD_GLOBAL)


def test_kernel_ops_registered_in_both_builds():
    import torch

    for name, ns in (("_hcb_kernels.so", "hcb"), ("_hcb_kernels_f16.so", "hcb16")):
        path = os.path.join(PKG, name)
        if not os.path.exists(path):
            pytest.skip(f"{name} not built")
        torch.ops.load_library(path)
        lib = getattr(torch.ops, ns)
        for op in ("conv_p3", "conv_p3_bnb", "conv_wgrad_p3", "conv_igemm", "bn_stats_acc", "set_deterministic",
                   "bn_bwd_apply_acc"):
            assert hasattr(lib, op), (ns, op)
