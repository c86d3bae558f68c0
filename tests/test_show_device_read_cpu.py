"""CPU: `show --device-read` is refused where it cannot work, before anything is created -- with `--host-draw` (status 2) and on
a machine without a GPU (status 1) -- and `draw_video` refuses parsed rows for the numpy path."""
import os

import pytest

from test_show_resident_cpu import _tree


def test_device_read_does_not_go_with_host_draw(tmp_path, capsys):
    from gomatching_amd import show
    data, out = _tree(tmp_path)
    drawn = str(tmp_path / "drawn")
    assert show.main(["--input", data, "--results", out, "--output", drawn, "--device-read", "--host-draw"]) == 2
    err = capsys.readouterr().err
    assert "--device-read" in err and "--host-draw" in err
    assert not os.path.exists(drawn)


def test_device_read_needs_a_gpu(tmp_path, capsys, monkeypatch):
    import torch
    from gomatching_amd import show
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (on a GPU machine too: the status of a machine without)
    data, out = _tree(tmp_path)
    drawn = str(tmp_path / "drawn")
    assert show.main(["--input", data, "--results", out, "--output", drawn, "--device-read"]) == 1
    assert "needs a GPU" in capsys.readouterr().err
    assert not os.path.exists(drawn)


def test_draw_video_refuses_parsed_rows_on_the_host_path(tmp_path):
    import numpy as np
    from gomatching_amd import results, show
    host = [np.zeros(3, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8),
            np.zeros(1, np.int32), np.zeros((0, 2), np.int32)]
    parsed = results.ParsedRows(0, None, host, [])
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    with pytest.raises(ValueError, match="drawn on the GPU"):
        show.draw_video(frames, None, ["1.jpg", "2.jpg"], "v", str(tmp_path), 37, None, show.Atlas(), host=True, parsed=parsed)
    with pytest.raises(show.ShowError, match="video v: 3 frames but results for 2"):
        show.draw_video(frames + frames[:1], None, ["1.jpg", "2.jpg", "3.jpg"], "v", str(tmp_path), 37, None, show.Atlas(),
                        parsed=parsed)
