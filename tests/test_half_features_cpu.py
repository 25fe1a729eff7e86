"""Half-precision feature entry points without a GPU: the typed twins are declared, exported and bound; the code object holds the typed
encoder kernels with zero scratch; ops refuses CPU half tensors like every other input."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
TYPED = ["snn_rpn_head_forward_stages_typed", "snn_rpn_head_forward_readouts_typed", "snn_det_head_forward_k_typed",
         "snn_det_head_forward_readouts_typed", "snn_det_head_forward_roialign_k_typed", "snn_det_head_forward_roialign_readouts_typed",
         "snn_encode_nchw_typed", "snn_roi_align_encode_typed"]


def test_typed_entry_points_are_declared_exported_and_bound():
    from snn_automotive_object_detection_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "snn_hip.h")).read()
    for n in TYPED:
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\bint %s\(" % n, hdr), n
    assert re.search(r"SNN_FEAT_F32 = 0, SNN_FEAT_F16 = 1, SNN_FEAT_BF16 = 2", hdr)
    assert _lib.FEAT_DTYPES == {"f32": 0, "f16": 1, "bf16": 2}
    assert int(re.search(r"#define SNN_STATUS_NO_TYPED_KERNEL (\d+)", hdr).group(1)) == _lib.NO_TYPED_KERNEL > 0


def test_typed_entries_validate_dtype_and_alignment_before_any_device_work():
    import ctypes as C
    from snn_automotive_object_detection_amd import _lib
    lib = _lib.load()
    p = _lib.snn_params(0.1, -0.2, 0, 0, 0.25, 0.1, 0, 0)
    assert lib.snn_encode_nchw_typed(C.c_void_p(4096), 7, 1, 32, 4, 4, 8, C.byref(p), C.c_void_p(4096), 16, None) == -1
    assert b"feat_dtype" in lib.snn_last_error()
    assert lib.snn_encode_nchw_typed(C.c_void_p(4098), 1, 1, 32, 4, 4, 8, C.byref(p), C.c_void_p(4096), 16, None) == -1
    assert b"16-byte aligned" in lib.snn_last_error()
    assert lib.snn_det_head_forward_k_typed(C.c_void_p(4104), 2, 1, 3136, 32, 3, 12, 8, C.byref(p), C.c_void_p(4096), 49, *([C.c_void_p(4096)] * 9),
                                            1 << 40, None) == -1
    assert b"16-byte aligned" in lib.snn_last_error()


def test_code_object_holds_the_typed_encoders_with_zero_scratch(tmp_path):
    if not (os.path.exists(READELF) and os.path.exists(OBJDUMP)):
        pytest.skip("no llvm-readelf / llvm-objdump")
    from snn_automotive_object_detection_amd import build as B
    subprocess.run(["cp", B.build(force=False), str(tmp_path / "lib.so")], check=True)
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL)
    objs = [f for f in os.listdir(str(tmp_path)) if "gfx950" in f]
    assert len(objs) == 1
    notes = subprocess.run([READELF, "--notes", objs[0]], cwd=str(tmp_path), check=True, stdout=subprocess.PIPE, text=True).stdout
    scratch = {}
    for blk in notes.split("- .agpr_count")[1:]:                       # one metadata record per kernel
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        scratch[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert len(scratch) >= 100
    for stem, n in (("k_encode_levels_h", 6), ("k_encode_nchw_h", 6), ("k_encode_rows_wm_h", 6), ("k_encode_rows_perm_h", 8),
                    ("k_roi_align_encode_tab_h", 2), ("k_roi_align_encode_perm_h", 2)):
        hits = [k for k in scratch if re.match(r"_Z\d+%sI" % stem, k)]
        assert len(hits) == n and all("feat_f16" in k or "feat_bf16" in k for k in hits), (stem, hits)
        assert all(scratch[k] == 0 for k in hits), {k: scratch[k] for k in hits}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_ops_refuses_cpu_half_tensors(dtype):
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import ops
    from snn_automotive_object_detection_amd._lib import SnnHipError
    p = ops.make_params(ops.LIFParameters(v_th=torch.as_tensor(0.25)), ops.LIFParameters(v_th=torch.as_tensor(0.1)))
    with pytest.raises(SnnHipError):
        S.RPNHeadSNN(32, 3, 4)([torch.randn(1, 32, 4, 4).to(dtype)])
    with pytest.raises(SnnHipError):
        S.FastRCNNPredictorSNNFull(49 * 8, 32, 3, 4)(torch.randn(2, 8, 7, 7).to(dtype))
    with pytest.raises(SnnHipError):
        ops.encode_nchw(torch.randn(1, 32, 4, 4).to(dtype), 4, p)
    with pytest.raises(SnnHipError):
        ops.roi_align_encode([torch.randn(1, 8, 4, 4).to(dtype)], [0.25], torch.zeros(2, 4), torch.zeros(2), torch.zeros(2), 4, p)
