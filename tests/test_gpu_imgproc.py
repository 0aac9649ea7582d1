"""GPU: pg_preprocess_images (include/plangen_hip.h) -- the reference's VLMImageProcessor on the device -- against the stored Pillow +
transformers fixture (tests/golden/imgproc_cases.npz, tools/make_imgproc_golden.py), bit for bit.  tests/imgproc_ref.py (checked against
the same fixture and against Pillow live in tests/test_imgproc_cpu.py) supplies the results the fixture stores as digests only and the
inputs the fixture does not cover."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import imgproc_ref as IR
from conftest import ROOT, get_engine
from plangen_amd import _lib

pytestmark = pytest.mark.gpu

IDS = [IR.case_name(*c) for c in IR.CASES]
ALL = IR.CASES + IR.EXTRA_CASES
ALL_IDS = [IR.case_name(*c) for c in ALL]
BG = IR.background_of(IR.CLIP_MEAN)
IDENTITY = np.broadcast_to(np.arange(256, dtype=np.float32), (3, 256)).copy()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "imgproc_cases.npz"))


@pytest.fixture(scope="module")
def ref():
    """Per case of CASES + EXTRA_CASES, computed once and left unchanged: (input uint8 HWC, padded uint8 [S, S, 3], final fp32 [3, S, S])."""
    out = []
    for i, (h, w, s) in enumerate(ALL):
        a = IR.case_input(i)
        out.append((a, IR.preprocess_u8(a, s, background=BG), IR.preprocess(a, s, IR.CLIP_MEAN, IR.CLIP_STD)))
    return out


@pytest.fixture(scope="module")
def eng(tiny_cfg, tiny_weights):
    return get_engine(tiny_cfg, tiny_weights, "f32")


def _want(golden, ref, idx):
    """(padded, final) the fixture holds for case idx, or (None, None) plus its digests."""
    n = ALL_IDS[idx]
    if idx < len(IR.CASES) and (n + "/padded") in golden.files:
        return golden[n + "/padded"], golden[n + "/final"], None
    return None, None, (list(golden[n + "/sha256"]) if idx < len(IR.CASES) else None)


def _check_u8(golden, ref, idx, got_chw):
    """got_chw: float [3, S, S] produced with the identity table == the fixture's resized and padded uint8 image."""
    assert not np.isnan(got_chw).any(), "an output element was not written"
    got = got_chw.transpose(1, 2, 0)
    assert np.array_equal(got, np.round(got)) and got.min() >= 0 and got.max() <= 255
    got = got.astype(np.uint8)
    padded, _, digests = _want(golden, ref, idx)
    diff = np.abs(got.astype(int) - ref[idx][1].astype(int))
    msg = f"{ALL_IDS[idx]}: {int((diff != 0).sum())} of {diff.size} values differ from imgproc_ref, max {int(diff.max())}"
    if padded is not None:
        assert np.array_equal(got, padded), msg
    elif digests is not None:
        assert _sha(got) == digests[2], msg
    assert np.array_equal(got, ref[idx][1]), msg


def _check_final(golden, ref, idx, got, bf16=False):
    _, final, digests = _want(golden, ref, idx)
    want = final if final is not None else ref[idx][2]
    if bf16:
        want_bits = torch.from_numpy(np.ascontiguousarray(want)).to(torch.bfloat16).view(torch.int16).numpy()
        got_bits = got.view(torch.int16).cpu().numpy()
        if digests is not None:
            assert _sha(got_bits) == digests[4]
        assert np.array_equal(got_bits, want_bits), ALL_IDS[idx]
    else:
        g = got.cpu().numpy()
        if digests is not None:
            assert _sha(g) == digests[3]
        assert g.dtype == np.float32 and np.array_equal(g.view(np.int32), np.ascontiguousarray(want).view(np.int32)), ALL_IDS[idx]


def _nan(eng, B, S, dtype=torch.float32):
    return torch.full((B, 3, S, S), float("nan"), dtype=dtype, device=eng.device)


@pytest.mark.parametrize("idx", range(len(ALL)), ids=ALL_IDS)
def test_identity_table_gives_the_resized_and_padded_uint8_image(eng, golden, ref, idx):
    s = ALL[idx][2]
    out = _nan(eng, 1, s)
    eng.preprocess_images([ref[idx][0]], s, IR.MIN_SIZE, background=BG, lut=IDENTITY, out=out)
    _check_u8(golden, ref, idx, out[0].cpu().numpy())


@pytest.mark.parametrize("idx", range(len(ALL)), ids=ALL_IDS)
def test_real_table_fp32_and_bf16_equal_the_fixture_bit_for_bit(eng, golden, ref, idx):
    s = ALL[idx][2]
    for dt in (torch.float32, torch.bfloat16):
        out = _nan(eng, 1, s, dt)
        got = eng.preprocess_images([ref[idx][0]], s, IR.MIN_SIZE, mean=IR.CLIP_MEAN, std=IR.CLIP_STD, dtype=dt, out=out)
        assert got is out and not torch.isnan(out).any()
        _check_final(golden, ref, idx, out[0], bf16=dt == torch.bfloat16)


def test_all_cases_in_one_call_equal_one_call_each(eng, golden, ref):
    for s in sorted({c[2] for c in ALL}):
        idxs = [i for i, c in enumerate(ALL) if c[2] == s]
        out = _nan(eng, len(idxs), s)
        eng.preprocess_images([ref[i][0] for i in idxs], s, IR.MIN_SIZE, mean=IR.CLIP_MEAN, std=IR.CLIP_STD, out=out)
        for k, i in enumerate(idxs):
            single = eng.preprocess_images([ref[i][0]], s, IR.MIN_SIZE, mean=IR.CLIP_MEAN, std=IR.CLIP_STD)
            assert torch.equal(out[k], single[0]), ALL_IDS[i]
            _check_final(golden, ref, i, out[k])


@pytest.mark.parametrize("idx", [0, 3, 6, 11], ids=[ALL_IDS[i] for i in (0, 3, 6, 11)])
def test_strided_view_of_a_wider_buffer_equals_the_contiguous_form(eng, golden, ref, idx):
    """Rows passed through row_stride, not copied: both passes, the copy-only case (both passes skipped) and the vertical-only case (its
    loads come straight from the source) on rows that start at odd addresses."""
    a = ref[idx][0]
    h, w, s = ALL[idx]
    wide = torch.full((h, w + 7, 3), 201, dtype=torch.uint8, device=eng.device)
    view = wide[:, 3:3 + w]
    view.copy_(torch.from_numpy(a))
    assert not view.is_contiguous() and view.stride(0) == (w + 7) * 3 and view.data_ptr() % 4 != 0
    out = _nan(eng, 1, s)
    eng.preprocess_images([view], s, IR.MIN_SIZE, background=BG, lut=IDENTITY, out=out)
    assert eng._keep[0].data_ptr() == view.data_ptr()                               # not copied
    _check_u8(golden, ref, idx, out[0].cpu().numpy())


def _raw(eng, descs, B, S, min_size, out, bg=BG, lut=IDENTITY, images_null=False, bg_null=False, lut_null=False, out_null=False, dtype=_lib.PG_F32):
    arr = (_lib.pg_image_u8 * max(1, len(descs)))()
    for d, (ptr, h, w, st) in zip(arr, descs):
        d.pix_dev, d.height, d.width, d.row_stride = ptr, h, w, st
    bgc = (C.c_uint8 * 3)(*bg)
    table = np.ascontiguousarray(lut, dtype=np.float32)
    return eng.lib.pg_preprocess_images(eng.h, None if images_null else arr, B, S, min_size, None if bg_null else bgc,
                                        None if lut_null else table.ctypes.data_as(C.POINTER(C.c_float)),
                                        C.c_void_p(0 if out_null else out.data_ptr()), dtype, eng.stream)


def test_every_argument_error_returns_pg_err_arg_and_launches_nothing(eng):
    S = 32
    img = torch.randint(0, 256, (40, 50, 3), dtype=torch.uint8, device=eng.device)
    ok = (img.data_ptr(), 40, 50, 150)
    out = torch.full((2, 3, S, S), -7.0, device=eng.device)
    bad = {
        "height 0": dict(descs=[ok, (img.data_ptr(), 0, 50, 150)], B=2),
        "width 0": dict(descs=[(img.data_ptr(), 40, 0, 150)], B=1),
        "negative side": dict(descs=[(img.data_ptr(), -3, 50, 150)], B=1),
        "S < min_size": dict(descs=[ok], B=1, S=8, min_size=14),
        "min_size 0": dict(descs=[ok], B=1, min_size=0),
        "ratio above 64 (width)": dict(descs=[ok, (img.data_ptr(), 40, 64 * S + 1, 3 * (64 * S + 1))], B=2),
        "ratio above 64 (height, against the clamped size)": dict(descs=[(img.data_ptr(), 64 * 14 + 1, 64 * S, 3 * 64 * S)], B=1),
        "B 0": dict(descs=[ok], B=0),
        "B negative": dict(descs=[ok], B=-1),
        "null image pointer": dict(descs=[ok, (None, 40, 50, 150)], B=2),
        "null descriptor array": dict(descs=[ok], B=1, images_null=True),
        "null background": dict(descs=[ok], B=1, bg_null=True),
        "null table": dict(descs=[ok], B=1, lut_null=True),
        "null output": dict(descs=[ok], B=1, out_null=True),
    }
    for name, kw in bad.items():
        kw = dict(kw)
        rc = _raw(eng, kw.pop("descs"), kw.pop("B"), kw.pop("S", S), kw.pop("min_size", 14), out, **kw)
        assert rc == -1, (name, rc)
        assert eng.lib.pg_last_error(eng.h), name
    assert eng.lib.pg_preprocess_images(None, None, 1, S, 14, None, None, None, 0, eng.stream) == -1      # null handle
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a rejected call wrote to the output"
    # the limits themselves are accepted: ratio exactly 64, S == min_size
    assert _raw(eng, [(img.data_ptr(), 1, 1, 3)], 1, 14, 14, out[:1, :, :14, :14].contiguous()) == 0
    big = torch.zeros((14, 64 * S, 3), dtype=torch.uint8, device=eng.device)
    assert _raw(eng, [(big.data_ptr(), 14, 64 * S, 3 * 64 * S)], 1, S, 14, out) == 0
    torch.cuda.synchronize()
    assert bool((out[0] == torch.tensor([0.0, 0.0, 0.0], device=eng.device).view(3, 1, 1)).logical_or(
        out[0] == torch.tensor([float(v) for v in BG], device=eng.device).view(3, 1, 1)).all())


def test_ratio_64_with_257_taps_equals_the_reference(eng):
    """The largest kernel the contract admits: 64 x down-scaling, 257 taps per output, horizontal blocks narrowed to what fits their LDS span."""
    S = 16
    rs = np.random.RandomState(77)
    a = rs.randint(0, 256, (20, 64 * S, 3)).astype(np.uint8)
    want = IR.preprocess_u8(a, S, background=BG)
    out = _nan(eng, 1, S)
    eng.preprocess_images([a], S, IR.MIN_SIZE, background=BG, lut=IDENTITY, out=out)
    got = out[0].cpu().numpy().transpose(1, 2, 0)
    assert not np.isnan(got).any() and np.array_equal(got.astype(np.uint8), want) and np.array_equal(got, np.round(got))


def test_two_calls_back_to_back_while_the_workspace_grows(tiny_cfg, tiny_weights, golden, ref):
    """A fresh engine: its first call allocates the workspace, the second (larger batch, larger images) outgrows it while the first may
    still be running; both are correct and pg_device_bytes counts the workspace."""
    from plangen_amd.engine import Engine
    e = Engine(tiny_cfg, dtype="f32", max_rows=2, max_prompt=16, max_images=1)
    try:
        b0 = e.device_bytes()
        small, large = [0], [3, 6, 7]                        # S = 32: one image; S = 48: three
        o1 = _nan(e, 1, 32)
        o2 = _nan(e, 3, 48)
        e.preprocess_images([ref[i][0] for i in small], 32, IR.MIN_SIZE, mean=IR.CLIP_MEAN, std=IR.CLIP_STD, out=o1)
        b1 = e.device_bytes()
        keep = e._keep
        e.preprocess_images([ref[i][0] for i in large], 48, IR.MIN_SIZE, mean=IR.CLIP_MEAN, std=IR.CLIP_STD, out=o2)
        b2 = e.device_bytes()
        torch.cuda.synchronize()
        del keep
        assert b0 < b1 < b2
        _check_final(golden, ref, 0, o1[0])
        for k, i in enumerate(large):
            _check_final(golden, ref, i, o2[k])
        o3 = _nan(e, 1, 32)                                  # a smaller batch afterwards reuses the grown workspace
        e.preprocess_images([ref[1][0]], 32, IR.MIN_SIZE, mean=IR.CLIP_MEAN, std=IR.CLIP_STD, out=o3)
        assert e.device_bytes() == b2
        _check_final(golden, ref, 1, o3[0])
    finally:
        e.close()


def test_processor_on_arrays_equals_the_fixture(eng, golden, ref):
    from plangen_amd.imageproc import VLMImageProcessor
    p = VLMImageProcessor(image_size=32, engine=eng)                                # class defaults: CLIP mean / std
    idxs = [i for i, c in enumerate(IR.CASES) if c[2] == 32]
    px = p([ref[i][0] for i in idxs], return_tensors="pt").pixel_values
    assert px.shape == (len(idxs), 3, 32, 32) and px.dtype == torch.float32 and px.is_cuda
    for k, i in enumerate(idxs):
        _check_final(golden, ref, i, px[k])
    Image = pytest.importorskip("PIL.Image")
    px1 = p(Image.fromarray(ref[idxs[0]][0], "RGB")).pixel_values
    _check_final(golden, ref, idxs[0], px1[0])
    raw = VLMImageProcessor(image_size=32, engine=eng, do_normalize=False)([ref[idxs[0]][0]]).pixel_values[0].cpu().numpy()
    want = IR.preprocess(ref[idxs[0]][0], 32, IR.CLIP_MEAN, IR.CLIP_STD, do_normalize=False)
    assert np.array_equal(raw.view(np.int32), want.view(np.int32))


def test_mmu_batch_from_image_path_rows_equals_image_pt_rows(tmp_path, tiny_cfg):
    """project/plangen: rows with ``image_path`` (.npy uint8 HWC) go through the device processor and yield the pixel_values and the
    greedy text ids of the same rows given as ``image_pt`` tensors computed by imgproc_ref."""
    import train
    from project.plangen.plangen_base import System as CliSystem
    S = tiny_cfg.vit_img
    half = (0.5, 0.5, 0.5)
    rs = np.random.RandomState(5)
    rows_path, rows_pt = [], []
    for i, (h, w) in enumerate([(50, 81), (90, 64)]):
        a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        np.save(str(tmp_path / f"im{i}.npy"), a)
        torch.save(torch.from_numpy(IR.preprocess(a, S, half, half)), str(tmp_path / f"im{i}.pt"))
        q = {"base_caption": f"red box {i} left of blue chair", "gt_grounding": "", "image_id": ""}
        rows_path.append(dict(q, image_path=str(tmp_path / f"im{i}.npy")))
        rows_pt.append(dict(q, image_pt=str(tmp_path / f"im{i}.pt")))
    f = tmp_path / "rows.jsonl"
    f.write_text("\n".join(json.dumps(r) for r in rows_path))
    opts = ["test=True", "tiny=True", "test_batch_size=2", "max_test_len=1", "dtype='f32'", "temperature=0.0", f"out_path={str(tmp_path)!r}",
            "test_data.task_type='mmu'", "max_new_tokens=8", "max_prompt=160", "synthetic=True"]
    a = train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", *opts])
    a.test_data = dict(a.test_data, data_file=str(f), data_name="imgs")
    m = CliSystem(a, None)
    try:
        dl = m.setup_data(None)
        m.resume(None)
        b_path, b_pt = dl[0], m.collate(rows_pt)
        px_a, px_b = b_path["prepare_inputs_infer"]["pixel_values"], b_pt["prepare_inputs_infer"]["pixel_values"]
        assert px_a.shape == px_b.shape == (2, 1, 3, S, S)
        assert torch.equal(px_a.float().cpu(), px_b.float().cpu())
        kw = dict(gen_path=str(tmp_path), save_local=False, max_new_tokens=8, pred_image=False, is_mmu=True)
        ids_a = m.uni_generate(batch=b_path, batch_idx="0", **kw)["pr_text_ids"]
        ids_b = m.uni_generate(batch=b_pt, batch_idx="1", **kw)["pr_text_ids"]
        assert ids_a.numel() > 0 and torch.equal(ids_a.cpu(), ids_b.cpu())
    finally:
        m.engine.close()
