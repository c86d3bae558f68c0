"""CPU: the flags of the resident drawing chain are refused where they cannot work, before anything is created --
`eval --online --show` without `--device-decode` and with `--host-draw`, `show --device-decode --host-draw`, `show --decode-walk`
alone (status 2), and `show --device-decode` on a machine without a GPU (status 1)."""
import json
import os

import numpy as np
from PIL import Image


def _tree(tmp_path):
    data = tmp_path / "ICDAR15_frames" / "Video_9_1_1"
    data.mkdir(parents=True)
    rng = np.random.RandomState(3)
    for i in range(2):
        Image.fromarray(rng.randint(0, 256, (40, 64, 3)).astype(np.uint8)).save(str(data / ("%d.jpg" % (i + 1))), quality=90)
    out = tmp_path / "out"
    (out / "jsons").mkdir(parents=True)
    obj = {"points": [5, 5, 50, 5, 50, 30, 5, 30], "ID": 4, "transcription": "abc",
           "segmentation": [[[5, 5], [50, 5], [50, 30], [5, 30]]]}
    with open(str(out / "jsons" / "Video_9_1_1.json"), "w") as fp:
        json.dump({"1": [obj], "2": []}, fp)
    return str(tmp_path / "ICDAR15_frames"), str(out)


def test_eval_online_show_is_refused_without_device_decode_and_with_host_draw(tmp_path, capsys):
    from gomatching_amd import eval as E
    data, _ = _tree(tmp_path)
    refused = str(tmp_path / "refused")
    base = ["--builtin", "icdar15", "--input", data, "--output", refused]
    assert E.main(base + ["--online", "--show"]) == 2
    err = capsys.readouterr().err
    assert "--device-decode" in err and "--show" in err                  # the refusal says what it does go with
    assert E.main(base + ["--online", "--show", "--device-decode", "--host-draw"]) == 2
    assert "--host-draw" in capsys.readouterr().err
    assert E.main(base + ["--online", "--show", "--device-encode"]) == 2
    assert not os.path.exists(refused)


def test_show_refuses_flags_that_do_not_go_together(tmp_path, capsys):
    from gomatching_amd import show
    data, out = _tree(tmp_path)
    drawn = str(tmp_path / "drawn")
    base = ["--input", data, "--results", out, "--output", drawn]
    assert show.main(base + ["--device-decode", "--host-draw"]) == 2
    assert "--host-draw" in capsys.readouterr().err
    assert show.main(base + ["--decode-walk", "chunks"]) == 2
    assert "--device-decode" in capsys.readouterr().err
    assert show.main(base + ["--decode-walk", "chunks", "--host-draw"]) == 2
    assert not os.path.exists(drawn)


def test_show_device_decode_needs_a_gpu(tmp_path, capsys, monkeypatch):
    import torch
    from gomatching_amd import show
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (on a GPU machine too: the status of a machine without)
    data, out = _tree(tmp_path)
    drawn = str(tmp_path / "drawn")
    assert show.main(["--input", data, "--results", out, "--output", drawn, "--device-decode"]) == 1
    assert "needs a GPU" in capsys.readouterr().err
    assert show.main(["--input", data, "--results", out, "--output", drawn, "--device-decode", "--decode-walk", "segments"]) == 1
    assert not os.path.exists(drawn)


def test_draw_video_takes_host_frames_as_before(tmp_path):
    """Without a provider and without a GPU `draw_video` does what it did: the numpy rule over a list of host frames."""
    from concurrent.futures import ThreadPoolExecutor
    from gomatching_amd import eval as E
    from gomatching_amd import show
    data, out = _tree(tmp_path)
    paths = E.frame_paths(os.path.join(data, "Video_9_1_1"))
    frames = [E.read_frame(p) for p in paths]
    with open(os.path.join(out, "jsons", "Video_9_1_1.json")) as fp:
        annotation = show.rows_of_json(json.load(fp))
    assert not show.is_resident(frames) and not show.is_resident(np.stack(frames))
    with ThreadPoolExecutor(max_workers=2) as pool:
        show.draw_video(frames, annotation, paths, "Video_9_1_1", str(tmp_path / "lib"), 37, pool, show.Atlas(), host=True,
                        encode="host")
    assert sorted(os.listdir(str(tmp_path / "lib" / "results" / "Video_9_1_1"))) == ["1.jpg", "2.jpg"]
