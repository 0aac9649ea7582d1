#!/usr/bin/env python3
"""What the mmu path's image pre-processing costs for one batch, on the device and on the host, in ONE process: 64 seeded uint8 images
(32 of 640 x 480 and 32 of 1024 x 768, H x W = 480 x 640 / 768 x 1024) -> [64, 3, 384, 384] fp32, Janus-Pro's mean = std = 0.5.
  device  pg_preprocess_images on images already in device memory: HIP events around the call, median of 20 after a warm-up; also the
          host -> device copy of the 64 images (what a loader that decodes on the host pays on top)
  host    the reference's statements (PIL.Image.resize BICUBIC, expand2square, rescale, normalize) per image, on 1 thread and on a pool
          of 16 threads, median of 5
The figure is recorded, not gated.  Writes a markdown report (default profiles/preprocess_cost.md) and checks first that both sides
produce the same bits.
usage: preprocess_cost.py [out.md]"""
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
from make_imgproc_golden import reference_pipeline
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "preprocess_cost.md")
S, HALF = 384, (0.5, 0.5, 0.5)
rs = np.random.RandomState(0)
imgs = [rs.randint(0, 256, ((480, 640, 3) if i % 2 == 0 else (768, 1024, 3))).astype(np.uint8) for i in range(64)]

eng = Engine(PlanGenConfig.tiny(), dtype="f32", max_rows=2, max_prompt=16, max_images=1)
dev = [torch.from_numpy(a).to(eng.device) for a in imgs]
kw = dict(mean=HALF, std=HALF)


def host_one(a):
    return reference_pipeline(a, S, 14, HALF, HALF)[2]


got = eng.preprocess_images(dev, S, 14, **kw).cpu().numpy()
same = all(np.array_equal(got[i].view(np.int32), host_one(imgs[i]).view(np.int32)) for i in (0, 1, 62, 63))
assert same, "device and host results differ"

out = torch.empty((64, 3, S, S), dtype=torch.float32, device=eng.device)
ms = []
for it in range(21):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.preprocess_images(dev, S, 14, out=out, **kw)
    e1.record()
    e1.synchronize()
    if it:
        ms.append(e0.elapsed_time(e1))
h2d = []
for it in range(6):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tmp = [torch.from_numpy(a).to(eng.device) for a in imgs]
    torch.cuda.synchronize()
    if it:
        h2d.append((time.perf_counter() - t0) * 1e3)


def host_batch(threads):
    t0 = time.perf_counter()
    if threads == 1:
        r = [host_one(a) for a in imgs]
    else:
        with ThreadPoolExecutor(threads) as ex:
            r = list(ex.map(host_one, imgs))
    np.stack(r)
    return (time.perf_counter() - t0) * 1e3


host = {}
for th in (1, 16):
    host_batch(th)
    host[th] = [host_batch(th) for _ in range(5)]

name = torch.cuda.get_device_name(0)
import PIL
lines = [
    "# Image pre-processing cost: device against host (tools/preprocess_cost.py)",
    "",
    f"64 seeded uint8 images (32 of 640 x 480, 32 of 1024 x 768) -> [64, 3, {S}, {S}] fp32, mean = std = 0.5, min_size 14.  Device and host",
    "results were compared bit for bit on four of the images before timing.  Recorded, not gated.",
    "",
    f"Machine: {name}; torch {torch.__version__}; Pillow {PIL.__version__}; numpy {np.__version__}; host threads available to the process: {len(os.sched_getaffinity(0))}.",
    "",
    "| side | what | ms per batch of 64 |",
    "|---|---|---|",
    f"| device | `pg_preprocess_images`, images resident in device memory, HIP events, median of 20 (min .. max) | {statistics.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f}) |",
    f"| device | host -> device copy of the 64 images (pageable memory, wall clock, median of 5) | {statistics.median(h2d):.2f} |",
    f"| host | Pillow + numpy, 1 thread, median of 5 (min .. max) | {statistics.median(host[1]):.1f} ({min(host[1]):.1f} .. {max(host[1]):.1f}) |",
    f"| host | Pillow + numpy, pool of 16 threads, median of 5 (min .. max) | {statistics.median(host[16]):.1f} ({min(host[16]):.1f} .. {max(host[16]):.1f}) |",
    "",
    f"Workspace the handle grew for this batch: {eng.device_bytes()} bytes in all for the tiny handle (tables + uint8 intermediates included).",
    "",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write("\n".join(lines))
print("\n".join(lines))
eng.close()
