"""CPU: the image pre-processing contract (include/plangen_hip.h, pg_preprocess_images).  tests/imgproc_ref.py -- the numpy restatement the
GPU tests compare against -- equals the stored Pillow + transformers fixture (tools/make_imgproc_golden.py) bit for bit, and Pillow run
live; the lookup table equals transformers' rescale + normalize; the ABI declares and binds the entry point."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import imgproc_ref as IR
from conftest import ROOT
from plangen_amd import _lib
from plangen_amd import imageproc as IP

GOLDEN = os.path.join(ROOT, "tests", "golden", "imgproc_cases.npz")
IDS = [IR.case_name(*c) for c in IR.CASES]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def ref_results():
    """imgproc_ref on every case, computed once: (input, resized, padded, final)."""
    out = []
    for i, (h, w, s) in enumerate(IR.CASES):
        a = IR.case_input(i)
        oh, ow = IR.target_size(h, w, s)
        r = IR.resize(a, oh, ow)
        out.append((a, r, IR.pad_square(r, s, IR.background_of(IR.CLIP_MEAN)), IR.preprocess(a, s, IR.CLIP_MEAN, IR.CLIP_STD)))
    return out


def test_fixture_is_small_and_complete(golden):
    assert os.path.getsize(GOLDEN) < 300 * 1024
    for n in IDS:
        assert (n + "/final") in golden.files or (n + "/sha256") in golden.files, n


def test_target_size_divides_then_multiplies_then_truncates():
    assert IR.target_size(64, 97, 48) == (31, 48)              # int(64 / 97 * 48) = int(31.67): the short side is truncated, not rounded to 32
    assert IR.target_size(5, 200, 32) == (14, 32) and IR.target_size(200, 5, 32) == (32, 14)      # min_size clamp
    assert IR.target_size(37, 53, 32) == (22, 32) and IR.target_size(640, 427, 384) == (384, 256)


@pytest.mark.parametrize("idx", range(len(IR.CASES)), ids=IDS)
def test_ref_equals_fixture_bit_for_bit(golden, ref_results, idx):
    n = IDS[idx]
    a, resized, padded, final = ref_results[idx]
    if (n + "/sha256") in golden.files:
        assert tuple(golden[n + "/shape"]) == resized.shape[:2]
        assert [_sha(a), _sha(resized), _sha(padded), _sha(final), _sha(_bf16_bits(final))] == list(golden[n + "/sha256"])
    else:
        assert np.array_equal(golden[n + "/input"], a)
        assert golden[n + "/resized"].shape == resized.shape and np.array_equal(golden[n + "/resized"], resized)
        assert np.array_equal(golden[n + "/padded"], padded)
        assert golden[n + "/final"].dtype == np.float32 and np.array_equal(golden[n + "/final"].view(np.int32), final.view(np.int32))


@pytest.mark.parametrize("idx", range(len(IR.CASES)), ids=IDS)
def test_ref_equals_pillow_live(ref_results, idx):
    Image = pytest.importorskip("PIL.Image")
    a, resized, _, _ = ref_results[idx]
    got = np.asarray(Image.fromarray(a, "RGB").resize((resized.shape[1], resized.shape[0]), Image.BICUBIC))
    assert np.array_equal(got, resized)


@pytest.mark.parametrize("k", range(len(IR.EXTRA_CASES)))
def test_one_pass_cases_equal_pillow_live(k):
    Image = pytest.importorskip("PIL.Image")
    h, w, s = IR.EXTRA_CASES[k]
    a = IR.case_input(len(IR.CASES) + k)
    oh, ow = IR.target_size(h, w, s)
    assert (oh == h) != (ow == w)                                                   # exactly one pass runs
    assert np.array_equal(np.asarray(Image.fromarray(a, "RGB").resize((ow, oh), Image.BICUBIC)), IR.resize(a, oh, ow))


def test_cases_reach_the_branches_they_are_there_for(ref_results):
    by = dict(zip(IDS, ref_results))
    up = by["20x20_32"][1]
    assert (up == 0).any() and (up == 255).any()                                    # negative lobes clip
    chk = by["333x500_384"][1]
    assert (chk == 0).mean() > 0.02 and (chk == 255).mean() > 0.02                    # heavy clipping at the production size
    for n in ("48x31_48", "31x48_48"):                                                # the resample is skipped: pad only
        assert by[n][1].shape == by[n][0].shape and np.array_equal(by[n][1], by[n][0])
    assert by["37x53_32"][1].shape == (22, 32, 3)                                   # pad difference 10; 53x37 pads on the other axis
    p = by["64x97_48"][2]
    bg = np.array(IR.background_of(IR.CLIP_MEAN), np.uint8)
    assert (p[:8] == bg).all() and (p[8 + 31:] == bg).all() and p.shape == (48, 48, 3)          # 17 rows of padding: 8 above, 9 below


@pytest.mark.parametrize("mean,std", [((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), (IR.CLIP_MEAN, IR.CLIP_STD)], ids=["half", "clip"])
def test_lut_equals_transformers_on_every_value(mean, std):
    T = pytest.importorskip("transformers.image_transforms")
    v = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (3, 256, 1)).copy()       # channels first
    x = T.rescale(image=v, scale=1.0 / 255.0, input_data_format="channels_first")
    want_rescaled = x[:, :, 0].copy()
    want = T.normalize(image=x, mean=mean, std=std, input_data_format="channels_first")[:, :, 0]
    for lut in (IP.make_lut(mean, std), IR.make_lut(mean, std)):
        assert lut.dtype == np.float32 and lut.shape == (3, 256)
        assert np.array_equal(lut.view(np.int32), np.ascontiguousarray(want, dtype=np.float32).view(np.int32))
    assert np.array_equal(IP.make_lut(mean, std, do_normalize=False).view(np.int32), want_rescaled.astype(np.float32).view(np.int32))


def test_header_declares_and_lib_binds_pg_preprocess_images():
    hdr = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    assert "image_processing_vlm.py:41-52,127-192" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+pg_preprocess_images\s*\(\s*pg_handle\s+h\s*,\s*const\s+pg_image_u8\s*\*", code)
    assert re.search(r"typedef\s+struct\s+pg_image_u8\s*\{\s*const\s+uint8_t\s*\*\s*pix_dev;\s*int32_t\s+height,\s*width;\s*int64_t\s+row_stride;\s*\}", code)
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    assert "pg_preprocess_images" in bound and len(bound["pg_preprocess_images"][1]) == 10
    import ctypes as C
    assert C.sizeof(_lib.pg_image_u8) == 24 and _lib.pg_image_u8.row_stride.offset == 16
    assert "pg_preprocess_images;" in open(os.path.join(ROOT, "plangen_amd", "csrc", "plangen_hip.map")).read()
    assert "imgproc.o" in open(os.path.join(ROOT, "plangen_amd", "csrc", "Makefile")).read()


def test_processor_has_the_reference_attributes_and_passes_tensors_through(tmp_path):
    p = IP.VLMImageProcessor(image_size=384)
    assert (p.image_size, p.min_size, p.rescale_factor, p.do_normalize) == (384, 14, 1.0 / 255.0, True)
    assert tuple(p.image_mean) == IR.CLIP_MEAN and tuple(p.image_std) == IR.CLIP_STD and p.background_color == (122, 116, 104)
    assert IP.VLMImageProcessor(image_size=8, image_mean=None).background_color == (127, 127, 127)
    t = torch.randn(2, 3, 8, 8)
    out = p(t, return_tensors="pt")
    assert out.pixel_values is t                                                    # hack_image_proc: untouched, no engine needed
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p([np.zeros((4, 4, 3), np.uint8)])
    (tmp_path / "preprocessor_config.json").write_text(
        '{"image_size": 384, "min_size": 14, "image_mean": [0.5, 0.5, 0.5], "image_std": [0.5, 0.5, 0.5], "rescale_factor": 0.00392156862745098, '
        '"do_normalize": true, "background_color": [127, 127, 127], "image_processor_type": "VLMImageProcessor", "processor_class": "VLChatProcessor"}')
    q = IP.VLMImageProcessor.from_config(str(tmp_path))
    assert q.image_size == 384 and list(q.image_mean) == [0.5] * 3 and q.background_color == (127, 127, 127)
    assert IP.VLMImageProcessor.from_config(str(tmp_path / "nowhere"), image_size=64).image_size == 64
