"""Camera-encoder test material (no tests here): random states in the key format of ``ptq_state.export_camera_state`` built from
tests/_pyramid_layers.py, and the CPU statement chain the deployed encoder is compared with -- ``stem_statement``, the oracle's
``residual_block`` per bottleneck, ``cam_heads_statement``."""
import numpy as np

from _pyramid_layers import W_RMS, act_step, conv1x1_state, conv3x3_state, relu_stats

GRID = {"xbound": [-16.0, 16.0, 1.0], "ybound": [-16.0, 16.0, 1.0], "zbound": [-3.0, 3.0, 6.0], "ddiscr": [2.0, 24.0, 8.0], "mode": "LID"}
TRUNK = (("layer1", 3, 64, 1), ("layer2", 4, 128, 2))              # layer, blocks, width, stride of the first block


def oracle(state):
    from oracle.spec_pyramid import OraclePyramid
    orc = OraclePyramid.__new__(OraclePyramid)
    orc.s = state
    return orc


def stem_state(rng, name="conv1", a_zp=0, sigma=1.0, bias_mean=0.3):
    """conv1 on an N(0, 1) image: sigma = std of the pre-activation; the bias moves 60 % of the outputs above zero"""
    code = rng.integers(0, 256, size=(64, 3, 7, 7), dtype=np.uint8)
    zw = rng.integers(110, 146, size=64).astype(np.float32)
    dw = (sigma / (np.sqrt(147.0) * W_RMS) * rng.uniform(0.67, 1.33, size=64)).astype(np.float32)
    bias = rng.normal(bias_mean * sigma, 0.3 * sigma, size=64).astype(np.float32)
    return {name + "/w_code": code, name + "/w_delta": dw, name + "/w_zp": zw, name + "/bias": bias,
            name + "/a_delta": act_step(sigma, a_zp, True), name + "/a_zp": np.float32(a_zp), name + "/a_off": np.bool_(False)}


def block_state(rng, name, cin, width, in_q, in_stats, zps, shortcut):
    """One QuantBottleneck of the camera trunk: 1x1 cin -> width, dense 3x3, 1x1 width -> 4 width; ``shortcut``: a 1x1 downsample module"""
    zp1, zp2, zpo = zps
    cout = 4 * width
    s = conv1x1_state(rng, name + ".conv1", cin, width, in_q, in_stats, zp1)
    q1 = (s[name + ".conv1/a_delta"], zp1)
    s.update(conv3x3_state(rng, name + ".conv2", width, width, q1, relu_stats(zp1), zp2))
    q2 = (s[name + ".conv2/a_delta"], zp2)
    sigma = float(np.sqrt(in_stats[1] ** 2 - in_stats[0] ** 2)) * float(in_q[0])          # the shortcut's spread
    s.update(conv1x1_state(rng, name + ".conv3", width, cout, q2, relu_stats(zp2), 0, sigma=sigma, a_off=True))
    if shortcut:
        s.update(conv1x1_state(rng, name + ".downsample", cin, cout, in_q, in_stats, 0, sigma=sigma, a_off=True))
        mean, std = 0.6 * sigma, float(np.sqrt(2.0)) * sigma
    else:
        mean, std = 0.3 * sigma + in_stats[0] * float(in_q[0]), float(np.sqrt(2.0)) * sigma
    s[name + "/a_delta"], s[name + "/a_zp"], s[name + "/a_off"] = act_step(std, zpo, True, mean), np.float32(zpo), np.bool_(False)
    return s


def camera_state(seed, final_dim=(32, 48), depth_bins=8, features=64, zero_points=True, grid=GRID, downsample=8):
    """A whole camera state.  ``zero_points``: every quantizer gets its own non-zero zero point (what min-max calibration never produces
    behind a ReLU, and what the kernels' rings and epilogues must still get right); False: 0 behind every ReLU as in a calibrated model."""
    rng = np.random.default_rng(seed)
    zp = (lambda: int(rng.integers(1, 24))) if zero_points else (lambda: 0)
    z0 = zp()
    s = stem_state(rng, a_zp=z0)
    q, stats, cin = (s["conv1/a_delta"], z0), relu_stats(z0), 64
    blocks = []
    for layer, count, width, stride in TRUNK:
        for i in range(count):
            name = f"{layer}.{i}"
            zps = (zp(), zp(), zp())
            s.update(block_state(rng, name, cin, width, q, stats, zps, shortcut=i == 0))
            q, stats, cin = (s[name + "/a_delta"], zps[2]), relu_stats(zps[2]), 4 * width
            blocks.append(name)
    s.update(conv1x1_state(rng, "depth_head", cin, depth_bins, q, stats, 131 if zero_points else 128, relu=False, sigma=2.0))
    s.update(conv1x1_state(rng, "image_head", cin, features, q, stats, 120 if zero_points else 128, relu=False))
    s["meta/module_names"] = np.array([k[:-len("/w_code")] for k in s if k.endswith("/w_code")])
    s["meta/block_names"] = np.array(blocks)
    s["meta/camera_encoder"] = np.array("Resnet101")
    s["meta/use_gt_depth"] = np.bool_(False)
    s["meta/downsample"] = np.int64(downsample)
    s["meta/features"], s["meta/depth_bins"] = np.int64(features), np.int64(depth_bins)
    s["meta/final_dim"] = np.asarray(final_dim, dtype=np.int64)
    for k in ("xbound", "ybound", "zbound", "ddiscr"):
        s["meta/grid/" + k] = np.asarray(grid[k], dtype=np.float64)
    s["meta/grid/mode"] = np.array(grid["mode"])
    return s


def statement_chain(state, imgs, taps=None):
    """(depth f32 [V, D, fH, fW], feats f32 [V, C, fH, fW]) of the CPU statements; ``taps`` receives uint8 codes [V, H, W, C] per name"""
    from quantv2x_amd import camera_encoder as ce
    wdeq, bias, q = ce.stem_constants(state)
    x = ce.stem_statement(imgs, wdeq, bias, *q)
    if taps is not None:
        taps["maxpool"] = x
    orc, xq = oracle(state), (np.float32(q[0]), int(q[1]))
    for layer, count, _, stride in TRUNK:
        for i in range(count):
            x, xq = orc.residual_block(f"{layer}.{i}", x, xq, stride if i == 0 else 1, ["conv1", "conv2", "conv3"], taps)
    return ce.cam_heads_statement(x, xq, state)


def images(seed, views, h, w, channels=3):
    return np.random.default_rng(seed).standard_normal((views, channels, h, w)).astype(np.float32)


def codes_of(t):
    """interior of a padded i8 map (device tensor or numpy) as uint8 codes"""
    o = t.cpu().numpy() if hasattr(t, "cpu") else t
    return (o[:, 1:-1, 1:-1].astype(np.int16) + 128).astype(np.uint8)
