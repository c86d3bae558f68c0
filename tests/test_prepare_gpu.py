"""GPU: `gom_quad_bezier_i32` (csrc/prepare.hip) against its plain-Python statement (prepare_statement.py) -- every output word,
no tolerance, no case left out: with integers where the rule has integers and unfused, once-rounded fp64 elsewhere (and no
trigonometry) the kernel can go all the way to the 16 integers.  Then the command as a fresh child process on the fixture
trees, device output against `--host-bezier` output byte for byte, and one `Trainer` step on a clip mapped from the converted
ICDAR15 tree: the training path the file exists for."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prepare_fixture as F
import prepare_statement as S
from clip_data_fixture import AUG_OPTS
from helpers import mini_cfg
from gomatching_amd import ops, prepare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device(quads, hw):
    return ops.quad_bezier(torch.tensor(quads).to(DEV), torch.tensor(hw).to(DEV)).cpu().numpy()        # (copies: the batch is read-only)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_kernel_equals_the_statement_at_wave_and_block_edges(n):
    quads, hw, _, ref = S.reference_batch()
    got = _device(quads[:n], hw[:n])
    assert got.dtype == np.int32 and got.shape == (n, 16)
    assert np.array_equal(got, ref[:n])


def test_kernel_equals_the_statement_on_the_mixed_batch():
    quads, hw, fam, ref = S.reference_batch()
    got = _device(quads, hw)
    counts = np.bincount(fam, minlength=len(S.FAMILIES))
    print({name: int(c) for name, c in zip(S.FAMILIES, counts)})
    bad = np.nonzero((got != ref).any(1))[0]
    print("quads that differ: %d of %d" % (bad.size, S.BATCH), {S.FAMILIES[f]: int(c) for f, c in enumerate(np.bincount(fam[bad], minlength=len(S.FAMILIES))) if c})
    assert bad.size == 0, [(S.FAMILIES[fam[b]], quads[b].tolist(), hw[b].tolist(), ref[b].tolist(), got[b].tolist()) for b in bad[:3]]
    assert (counts >= S.BATCH // len(S.FAMILIES)).all()
    assert np.array_equal(prepare.quad_bezier_device(quads, hw), ref)              # the command's one upload, launch and copy


def test_op_rejects_what_the_kernel_cannot_take():
    q = torch.zeros(4, 8, dtype=torch.int32, device=DEV)
    hw = torch.ones(4, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.quad_bezier(q.cpu(), hw)
    with pytest.raises(ValueError):
        ops.quad_bezier(q.to(torch.int64), hw)
    with pytest.raises(ValueError):
        ops.quad_bezier(q[:, :6], hw)
    with pytest.raises(ValueError):
        ops.quad_bezier(q, hw[:3])
    with pytest.raises(ValueError):
        ops.quad_bezier(torch.zeros(4, 16, dtype=torch.int32, device=DEV)[:, ::2], hw)      # not contiguous


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return F.build_tree(str(tmp_path_factory.mktemp("prepare_raw")))


def _child(args):
    r = subprocess.run([sys.executable, "-m", "gomatching_amd.prepare"] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", ["icdar15", "dstext", "bovtext"])
def test_command_device_and_host_bezier_write_the_same_bytes(tree, tmp_path, name):
    dev, host = str(tmp_path / "device.json"), str(tmp_path / "host.json")
    args = [name, "--annotations", tree[name][0], "--frames", tree[name][1], "--output"]
    _child(args + [dev])
    assert prepare.main(args + [host, "--host-bezier"]) == 0
    got = _bytes(dev)
    assert got == _bytes(host) and b'"bezier_pts"' in got
    if name == "icdar15":                                         # `bezier` on an existing json: the reference's own file
        src, dev2, host2 = str(tmp_path / "ref.json"), str(tmp_path / "device2.json"), str(tmp_path / "host2.json")
        with open(src, "wb") as f:
            f.write(F.reference_json(name))
        _child(["bezier", "--json", src, "--output", dev2])
        assert prepare.main(["bezier", "--json", src, "--output", host2, "--host-bezier"]) == 0
        assert _bytes(dev2) == _bytes(host2) and b'"bezier_pts"' in _bytes(dev2)


def test_trainer_steps_on_a_clip_of_the_converted_tree(tree, tmp_path):
    from gomatching_amd import data
    from gomatching_amd.config import merge_from_list
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.solver import Trainer
    from gomatching_amd.synth import TRAINING_CLS_BIAS
    from gomatching_amd.weights import synth_state_dict
    ann, frames = tree["icdar15"]
    out = str(tmp_path / "train.json")
    doc = prepare.convert_icdar15(ann, frames)
    assert prepare.add_bezier(doc) == (len(doc["annotations"]), 0)                  # on the device
    with open(out, "w", encoding="utf-8") as f:
        f.write(prepare.dumps(doc))
    cfg = mini_cfg("icdar15", device="cuda")
    merge_from_list(cfg, AUG_OPTS)
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.0
    cfg.SOLVER.WARMUP_ITERS = 0
    assert cfg.MODEL.ROI_HEADS.WITH_RESR
    videos = data.get_video_dataset_dicts([data.load_video_json(out, frames)])
    video = [v for v in videos if os.path.basename(os.path.dirname(v["images"][0]["file_name"])) == "Video_5_2_0"][0]
    clip = data.GoMDatasetMapper(cfg, True)(video, np.random.default_rng(5))
    assert len(clip) == 3 and sum(fr["instances"]["gt_boxes"].shape[0] for fr in clip) >= 3
    assert all("polyline" in fr["instances"] for fr in clip)
    model = GoMatching(cfg, synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS), device=DEV)
    trainer = Trainer(cfg, model, str(tmp_path))
    h = trainer.step(clip)
    print({k: v for k, v in h.items()})
    assert {"loss_long_asso", "loss_short_asso", "loss_res", "total_loss"} <= set(h)
    assert all(np.isfinite(h[k]) for k in h) and h["iteration"] == 1
    model.close()
