"""The host-side helpers every deployed engine shares (quantv2x_amd/engine.py, engine_pyramid.py): scene layout of a model call, the
output dict's head slices, the heterogeneous Pyramid model's modality codes.  No GPU needed."""
import numpy as np
import pytest
import torch


def test_scene_layout_one_scene_and_several():
    from quantv2x_amd.engine import scene_layout
    pw = torch.eye(4, dtype=torch.float32).expand(1, 3, 3, 4, 4)                    # float32, not contiguous
    got, lens = scene_layout({"pairwise_t_matrix": pw, "record_len": torch.tensor([7])}, 3)
    assert lens == [3] and got.dtype == torch.float64 and got.is_contiguous() and torch.equal(got, pw.double())
    pw3 = torch.zeros((3, 2, 2, 4, 4), dtype=torch.float64)
    for rl in (torch.tensor([2, 1, 2]), [2, 1, 2], np.array([2, 1, 2])):
        got, lens = scene_layout({"pairwise_t_matrix": pw3, "record_len": rl}, 5)
        assert got is pw3 and lens == [2, 1, 2] and all(type(v) is int for v in lens)


def test_split_heads_are_views_of_the_stacked_predictions():
    from quantv2x_amd.engine import split_heads
    preds = torch.arange(2 * 9 * 3 * 4, dtype=torch.float32).reshape(2, 9, 3, 4).clone()
    out = split_heads(preds, [2, 5, 2])
    assert list(out) == ["cls_preds", "reg_preds", "dir_preds", "preds_tensor"] and out["preds_tensor"] is preds
    for k, (lo, hi) in {"cls_preds": (0, 2), "reg_preds": (2, 7), "dir_preds": (7, 9)}.items():
        assert torch.equal(out[k], preds[:, lo:hi]), k
        assert out[k].untyped_storage().data_ptr() == preds.untyped_storage().data_ptr() and out[k]._base is preds, k
    single = split_heads(preds, [2, 5, 2], "_single")
    assert list(single) == ["cls_preds_single", "reg_preds_single", "dir_preds_single"]
    assert all(v._base is preds for v in single.values())


def test_modality_codes_map_onto_names():
    from quantv2x_amd.engine_pyramid import modality_names_of
    names = ["m1", "m2", "m3"]
    assert modality_names_of(torch.tensor([1, 3, 2]), names) == ["m1", "m3", "m2"]
    assert modality_names_of([2, np.int64(1), 3.0], names) == ["m2", "m1", "m3"]
    assert modality_names_of(["m2", "m1"], names) == ["m2", "m1"]
    assert modality_names_of(("m9",), names) == ["m9"]                             # (an unknown name is the engines' to refuse)


@pytest.mark.parametrize("aml,code", [([1, 0], "0"), (torch.tensor([4]), "4"), ([-1], "-1"), ([2.0, 5.0], "5.0")])
def test_modality_codes_out_of_range_are_refused(aml, code):
    from quantv2x_amd.engine_pyramid import modality_names_of
    with pytest.raises(ValueError, match=rf"modality code {code} outside 1\.\.3"):
        modality_names_of(aml, ["m1", "m2", "m3"])


@pytest.mark.parametrize("aml", [[True], [1, False], torch.tensor([True, True]), [np.bool_(True)]])
def test_modality_codes_refuse_bools(aml):
    from quantv2x_amd.engine_pyramid import modality_names_of
    with pytest.raises(ValueError, match="neither a modality name nor a code"):
        modality_names_of(aml, ["m1", "m2"])
