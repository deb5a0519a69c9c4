"""Shared by tests/test_camera_pyramid_cpu.py and tests/test_hip_bev_entry.py: a synthetic PTQ state of one QuantBasicBlock's input side
(conv1 with its quantizer, optionally the 1x1 downsample) and fp32 BEV maps as a lift-splat leaves them."""
import numpy as np

BLOCK = "backbone_m2.resnet.layer0.0"
ZP = 7                       # a non-zero output zero point: the ReLU's clamp is then not the conversion's saturation
X_STD = 1.5
SENT = -77                   # what the pad ring of a destination holds before the launch
# (n, cin, H, W, stride): a map smaller than a tile, odd sizes under stride 2, tile seams (33 and 17 columns), K = 720 (no power of two)
SHAPES = [(2, 16, 1, 1, 1), (1, 32, 5, 7, 2), (2, 80, 17, 33, 1), (2, 80, 17, 33, 2), (1, 64, 20, 20, 2)]
COUT = 64


def block_state(cin, cout, downsample, seed):
    """PTQ entries of BLOCK.conv1 (+ BLOCK.downsample): random weight codes, per-channel (delta, zp), a bias, conv1's quantizer sized so
    that the codes of a unit-variance-ish sum spread over the whole range and both clamps decide some"""
    rng = np.random.default_rng(seed)
    s = {}

    def module(name, k, a_off, a_delta):
        s[name + "/w_code"] = rng.integers(0, 256, size=(cout, cin, k, k), dtype=np.uint8)
        s[name + "/w_zp"] = rng.integers(110, 146, size=cout).astype(np.float32)
        s[name + "/w_delta"] = (rng.uniform(0.5, 1.5, size=cout) / (74.0 * np.sqrt(k * k * cin))).astype(np.float32)
        s[name + "/bias"] = (rng.standard_normal(cout) * 0.3).astype(np.float32)
        s[name + "/a_delta"], s[name + "/a_zp"], s[name + "/a_off"] = np.float32(a_delta), np.float32(0.0 if a_off else ZP), np.bool_(a_off)
    # sum of K products x * (code - zp) * dw: std about X_STD * 74 * sqrt(K) * dw = X_STD * (0.5 .. 1.5); 255 codes over about five of them
    module(BLOCK + ".conv1", 3, False, 5.0 * X_STD / 255.0)
    if downsample:
        module(BLOCK + ".downsample", 1, True, 1.0)
    return s


def bev_map(n, cin, h, w, seed):
    """f32 [n, cin, h, w] with both signs; whole channels and a corner region of exact zeros (cells no frustum point reaches), and one row
    scaled so that its sums clamp at both ends of the quantizer"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, cin, h, w)) * X_STD).astype(np.float32)
    x[:, 3::7] = 0.0
    x[:, :, : h // 2, : w // 3] = 0.0
    x[:, :, h - 1, :] *= np.float32(6.0)
    return x


def padded_i8(codes_u8, fill=SENT):
    """u8 [n, h, w, c] -> the device form: i8 [n, h + 2, w + 2, c] = code - 128 inside, ``fill`` on the ring"""
    n, h, w, c = codes_u8.shape
    out = np.full((n, h + 2, w + 2, c), fill, np.int8)
    out[:, 1:-1, 1:-1] = (codes_u8.astype(np.int16) - 128).astype(np.int8)
    return out
