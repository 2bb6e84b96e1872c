"""gpu: apply_r.main --resident - the analysis on the tables where the embedding wrote them - writes what the --render run writes, and never
brings the image table to the host."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARRAYS = ("cluster_centroids", "cluster_average_faces", "fixed_faces", "attributes", "attributes_fixer", "similar_by_attributes",
          "similar_by_pixels", "anomaly_distances", "variations")


def run_pair(tmp_path, monkeypatch, synthetic, n, batch):
    from ganrev import apply_r, nn_utils
    c, h, w, _ = (int(v) for v in synthetic.split("x"))
    downloads = []
    inner = nn_utils.DeviceTensor.numpy

    def recorder(self):
        downloads.append(self.size)
        return inner(self)
    a, b = str(tmp_path / "resident"), str(tmp_path / "render")
    args = ["--synthetic", synthetic, "--nbImages", str(n), "--batchSize", str(batch), "--quiet"]
    with monkeypatch.context() as mp:
        mp.setattr(nn_utils.DeviceTensor, "numpy", recorder)
        s1 = apply_r.main(args + ["--resident", "--writeTo", a])
    assert downloads and max(downloads) < n * c * h * w, (max(downloads), n * c * h * w)      # the image table stayed on the device
    s0 = apply_r.main(args + ["--render", "--writeTo", b])
    assert s1["path"] == "device-resident" and s0["path"] == "device"
    assert json.load(open(os.path.join(a, "summary.json")))["path"] == "device-resident"
    for key in ("cluster_sizes", "cluster_total_counts", "anomaly_below", "anomalies", "dims", "noiseDim", "nbImages"):
        assert s1[key] == s0[key], key
    assert not [f for f in os.listdir(a) if f.endswith(".png")]
    assert sorted(f for f in os.listdir(a)) == sorted(f for f in os.listdir(b) if not f.endswith(".png"))       # all of today's files
    for name in ARRAYS:
        fa, fb = os.path.join(a, name + ".npy"), os.path.join(b, name + ".npy")
        assert open(fa, "rb").read() == open(fb, "rb").read(), name
    assert any(s1["cluster_sizes"]) and np.load(os.path.join(a, "cluster_average_faces.npy")).shape == (20, c, h, w)


def test_resident_run_is_the_render_run(tmp_path, monkeypatch):
    run_pair(tmp_path, monkeypatch, "1x32x32x32", 600, 64)


def test_resident_run_rgb_nd100(tmp_path, monkeypatch):
    run_pair(tmp_path, monkeypatch, "3x64x64x100", 520, 64)
