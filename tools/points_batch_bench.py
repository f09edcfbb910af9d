#!/usr/bin/env python3
"""The export pipeline of the adapter header on device batches against the same pipeline on host vectors, in one process,
output bytes checked equal in the run (tests/cpp/points_batch_adapter.cc, built and run by this tool).

Pipeline, over four scans of one message shape (64 x 1024 and 128 x 2048, with intensities), streamed three times as the
outlier remover needs: assemble -> min_max_range_filter (1, 60 m) -> fixed_ratio_sampler (0.55) -> outlier removal
(mark hits / count rays / filter) -> intensity_to_color (0, 255) -> write_xray_image -> write_ply.

  (a) device batches: AssemblePointsBatch(kOnDevice, ...) and the adapter's processors; the batch stays in HBM
  (b) host vectors: AssemblePointsBatch's host vectors through the adapter's processors as they stood before batches
      lived on the device (kept_index downloads, KeepPoints, colours uploaded per insert), with the reference's sampler
      and PLY loops in C++ for the two stages that had no device form
  (c) the CPU model's sampler and PLY loops alone (tests/cpp/points_batch_model.cc, one thread)

Medians of --repeats warm passes over the whole pipeline, timed inside the C++ program.  Prints one JSON line a drive;
--out writes them to a file (profiles/points_batch_bench.json)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import points_batch_common as pb  # noqa: E402

RATIO = 0.55
f32 = np.float32


def bench(exe, model, directory, beams, azimuths, repeats):
    times, poses, mount, messages = pb.pipeline_messages(beams, azimuths)
    out = pb.run_adapter(exe, directory, times, poses, mount, messages, max_range=60.0, ratio=RATIO, repeats=repeats)
    assert out["device"][0] == out["host"][0] and out["device"][1].tobytes() == out["host"][1].tobytes(), "device batches differ"
    assert out["uploads"] == 0 and out["downloaded"] == out["records"]
    n = out["records"] // 19
    pulses = sum(len(m[1]) for m in messages)
    rng = np.random.RandomState(1)
    pts, it, col = rng.normal(size=(n, 3)).astype(f32), rng.uniform(0, 255, n).astype(f32), rng.uniform(0, 1, (n, 3)).astype(f32)
    _, sampler_seconds = pb.run_model(model, [pb.pulse_op(RATIO, 0, 0, pulses)], directory, timing=True)
    _, ply_seconds = pb.run_model(model, [pb.pack_op(pts, it, col, pb.PLY, 1, 1)], directory, timing=True)
    return dict(tool="points_batch_bench", beams=beams, azimuths=azimuths, scans=len(messages), points_per_scan=len(messages[0][1]),
                points_written=n, ply_record_bytes=out["records"], equal_to_host_path=True, cloud_uploads_device_path=out["uploads"],
                batch_bytes_downloaded_device_path=out["downloaded"], device_batches_ms=out["device_ms"],
                host_vectors_ms=out["host_ms"], host_over_device=out["host_ms"] / out["device_ms"],
                model_sampler_ms_per_phase=1e3 * sampler_seconds, model_ply_loop_ms=1e3 * ply_seconds, repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--out")
    args = ap.parse_args()
    import dliom as dl
    lines = []
    with tempfile.TemporaryDirectory() as directory:
        model = pb.build_model(directory)
        exe = pb.build_adapter(directory, dl.LIB_PATH)
        for beams, azimuths in ((64, 1024), (128, 2048)):
            lines.append(bench(exe, model, directory, beams, azimuths, args.repeats))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
