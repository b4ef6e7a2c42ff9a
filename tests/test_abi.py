"""The C-ABI library builds for gfx950, loads without a GPU and exports exactly what include/rangedet_hip.h declares;
the product loader fails loudly when the extension is missing (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from rangedet_amd import lib as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    h = open(os.path.join(ROOT, "include", "rangedet_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return sorted(set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", h)))


def test_header_and_binding_agree():
    assert _declared() == sorted(R.SIGNATURES)


def test_product_library_loads_and_exports_every_symbol():
    from rangedet_amd import build
    path = build.build(verbose=False)
    L = R.Lib(path)  # resolves every declared symbol (AttributeError otherwise)
    assert L.raw("rd_version")() >= 100
    # host-only entry points work without a GPU
    TAIL = 256                                                  # zero tail every packed buffer ends with (k_conv.h RD_CONV_TAIL)
    assert L.raw("rd_conv_packed_bytes")(9, 128, 128, R.RD_BF16) == 2 * 9 * 128 * 128 + TAIL
    assert L.raw("rd_conv_packed_bytes")(9, 72, 128, R.RD_BF16) == 2 * 9 * 128 * 128 + TAIL   # 72 -> two 64-channel chunks
    assert L.raw("rd_conv_packed_bytes")(1, 8, 64, R.RD_F32) == 64 * 128 + TAIL
    # every phase of the graph transposed convs: 6 taps (3 rows x 2 adjacent columns), run as a 6-step unit
    assert [L.raw("rd_deconv_phase_taps")(3, 8, 4, 2, p) for p in range(4)] == [6, 6, 6, 6]
    assert [L.raw("rd_deconv_phase_taps")(3, 4, 2, 1, p) for p in range(2)] == [6, 6]
    assert L.raw("rd_deconv_phase_taps")(3, 8, 4, 2, 4) == R.RD_EINVAL
    d = np.array([[0] * 11 + [s] for s in (0.7, 0.9, 0.7, 0.8)], np.float32)
    assert L.wnms_order_host(d).tolist()[:2] == [1, 3]
    assert L.raw("rd_meta_packed_bytes")(R.RD_BF16) == 36864 + 73728 + 2 * 2304 + 512 + 512 + 1024   # ... + the hidden layer as an MFMA fragment


def test_release_library_reads_no_environment():
    """Round 6: the library's code paths do not depend on the environment of the process -- it has no development
    switches and only one build -- and the Python-side lowering switches are ignored unless RD_DEV_SWITCHES=1 (rangedet_amd/devswitch.py).
    Checked on the binary: it does not even import getenv."""
    import subprocess
    from rangedet_amd import build, devswitch
    path = build.build(verbose=False)
    syms = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\b(secure_)?getenv\b", syms), "the release library imports getenv"
    # the Python side: a lowering switch without the master switch is not seen
    old = {k: os.environ.pop(k, None) for k in ("RD_DEV_SWITCHES", "RD_NO_FUSE_BLOCK")}
    try:
        os.environ["RD_NO_FUSE_BLOCK"] = "1"
        assert devswitch.get("RD_NO_FUSE_BLOCK") is None
        os.environ["RD_DEV_SWITCHES"] = "1"
        assert devswitch.get("RD_NO_FUSE_BLOCK") == "1"
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_missing_extension_fails_loudly(tmp_path):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.Lib(str(tmp_path / "librangedet_hip.so"))


def test_product_never_imports_oracle_or_emu():
    bad = []
    for dp, _, fs in os.walk(os.path.join(ROOT, "rangedet_amd")):
        for f in fs:
            if f.endswith((".py", ".h", ".hip")):
                t = open(os.path.join(dp, f)).read()
                if re.search(r"^\s*(from|import)\s+(oracle|emu_util)\b", t, re.M) or "librangedet_emu" in t or "liboracle" in t:
                    bad.append(f)
    assert not bad, bad


def test_no_gpu_means_no_run():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from rangedet_amd.runtime import TorchAllocator
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TorchAllocator()
