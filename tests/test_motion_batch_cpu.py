"""Motion clips as one padded batch, host side: the batch form of `DeepSolo.valid_shapes` against the per-frame function, the
oracle's padding masks and torch's nearest-neighbour resampling; `python -m gomatching_amd.train --motion-batch` argument
handling.  No GPU."""
import pytest
import torch

# (padded size, frame sizes): a full frame among padded ones; (8, 8) leaves ONE valid row and column on the coarse levels
SETS = [((96, 96), [(96, 96), (84, 96), (96, 96), (60, 80), (8, 8)]),
        ((72, 136), [(72, 136), (33, 136), (72, 41)])]
LEVELS = {(96, 96): [(12, 12), (6, 6), (3, 3), (2, 2)], (72, 136): [(9, 17), (5, 9), (3, 5), (2, 3)]}


@pytest.mark.parametrize("padded,sizes", SETS, ids=["96x96", "72x136"])
def test_batch_valid_shapes_equal_the_per_frame_function_and_the_padding_masks(padded, sizes):
    from gomatching_amd.modeling.deepsolo import DeepSolo
    from oracle import gom_oracle as O
    shapes = DeepSolo.level_shapes(*padded)
    assert shapes == LEVELS[padded]
    got = DeepSolo.valid_shapes_frames(shapes, sizes)
    assert len(got) == len(sizes) and all(len(v) == 4 for v in got)
    assert got == [DeepSolo.valid_shapes(shapes, hw) for hw in sizes]
    masks = O.mask_out_padding([(len(sizes), 256, h, w) for h, w in shapes[:3]], sizes)
    for b in range(len(sizes)):
        for l in range(3):
            free = ~masks[l][b]
            assert got[b][l] == (int(free.any(1).sum()), int(free.any(0).sum())), (b, l)
            assert bool(free[:got[b][l][0], :got[b][l][1]].all()) and int(free.sum()) == got[b][l][0] * got[b][l][1]
        # the extra level: nearest-neighbour resampling of level 0's mask (detection_transformer_wobackbone.py:177-178)
        m3 = torch.nn.functional.interpolate(masks[0][b][None, None].float(), size=shapes[3])[0, 0].bool()
        free = ~m3
        assert got[b][3] == (int(free.any(1).sum()), int(free.any(0).sum())), b
        assert int(free.sum()) == got[b][3][0] * got[b][3][1]
    assert got[0] == [tuple(s) for s in shapes]                   # the frame that fills the padded size: its full extents
    if (8, 8) in sizes:
        assert got[sizes.index((8, 8))][2:] == [(1, 1), (1, 1)]


def test_motion_batch_whole_needs_image_motion(capsys):
    from gomatching_amd import train
    assert train.get_parser().parse_args([]).motion_batch == "grouped"
    assert train.get_parser().parse_args(["--image-motion", "--motion-batch", "whole"]).motion_batch == "whole"
    assert train.main(["--builtin", "icdar15", "--motion-batch", "whole"]) == 2
    assert "--image-motion" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        train.main(["--builtin", "icdar15", "--image-motion", "--motion-batch", "halves"])
    assert e.value.code == 2
