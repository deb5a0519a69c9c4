"""tests/golden/codebook_seg_i8grid.npz: the reference's own ``UMGMQuantizer.encode`` (codebook.py:106-131, 231-239, 330-337) at
``(seg_num, dict_size)`` = (2, 256) and (1, 256) on rows that lie on the int8 grid -- the 35 200 rows of codebook_full.npz (its 8 800 real
rows, their channels rotated by 0 / 64 / 128 / 192, dequantized with its ``in_delta`` / ``in_zp``), which the candidate stage of the
two-stage exact encode can take (codebook_seg.npz pins these shapes on float rows).

Run in the build container only (the reference tree is imported through ``_refimport``, by way of ``make_golden``'s model builders):
``python tests/golden/make_golden_seg_i8grid.py``.  ONE BLAS thread: the reference's decision on near-ties depends on its thread order.
Arrays only: per shape ``codes_m{m}_k{k}`` u8 [levels * m][35200] (plane l * m + s) and ``gaps_m{m}_k{k}`` f16 [levels * m][35200], the
reference's top-2 distance gap per plane, rounded to half precision WITHOUT moving any gap across the 1e-4 the tests compare it with."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import _refimport  # noqa: E402,F401
import make_golden as MG  # noqa: E402

TAU = np.float32(1e-4)


def half_keeping_side(gaps):
    h = gaps.astype(np.float16)
    lo = np.float16(TAU)
    while np.float32(lo) > TAU:
        lo = np.nextafter(lo, np.float16(0))                             # the largest half <= 1e-4
    hi = np.nextafter(lo, np.float16(1))
    h = np.where((gaps <= TAU) & (h.astype(np.float32) > TAU), lo, h)
    h = np.where((gaps > TAU) & (h.astype(np.float32) <= TAU), hi, h)
    assert np.array_equal(h.astype(np.float32) > TAU, gaps > TAU)
    return h.astype(np.float16)


def main():
    from _common import calibrated_plugin
    from quantv2x_amd.ptq_state import export_ptq_state, extended_codebook
    torch.set_num_threads(1)
    g = np.load(os.path.join(HERE, "codebook_full.npz"))
    codes_u8 = np.concatenate([np.roll(g["rows_u8_real"], 64 * j, axis=1) for j in range(4)])
    rows = (codes_u8.astype(np.float32) - np.float32(g["in_zp"])) * np.float32(g["in_delta"])
    out = {"rows": np.int64(len(rows)), "tau": TAU}
    for m, k in ((2, 256), (1, 256)):
        cb = MG.build_ref(dict_size=k, seg_num=m).codebook
        state = export_ptq_state(calibrated_plugin("tiny", dict_size=k, seg_num=m))
        for l, enc in enumerate(cb._encoders):                           # the tests take the codebook from the seeded tiny state
            assert np.array_equal(extended_codebook(MG.np32(enc._quantizer._codebook)), state[f"codebook/{l}/codebook"]), l
        with torch.no_grad():
            xt = torch.from_numpy(rows)
            codes = cb.encode(xt)                                        # levels x [n, m]
            out[f"codes_m{m}_k{k}"] = np.concatenate([MG.np32(c).T for c in codes]).astype(np.uint8)
            cur, gaps = xt, []
            for enc in cb._encoders:
                z = enc._latentStageEncoder(cur)
                d = enc._quantizer._distance(enc._quantizationHead(z))   # [n, m, k]
                top2 = torch.topk(d, 2, dim=-1, largest=False)[0]
                gaps.append(MG.np32(top2[..., 1] - top2[..., 0]).T)
                cur, _ = enc.encode(cur)
            gaps = np.concatenate(gaps).astype(np.float32)
            out[f"gaps_m{m}_k{k}"] = half_keeping_side(gaps)
            print((m, k), out[f"codes_m{m}_k{k}"].shape, "planes with a gap <= 1e-4:", int((gaps <= TAU).sum()), "of", gaps.size)
    path = os.path.join(HERE, "codebook_seg_i8grid.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
