"""Random layer states of the Pyramid model's layer kinds in the ``ptq_state`` key format (no tests here).

``name/w_code`` u8, ``w_delta`` / ``w_zp`` / ``bias`` per output channel, ``a_delta``, ``a_zp``, ``a_off``: what ``OraclePyramid.q`` and the
engine's packers (``_Conv1x1``, ``_GConv``, ``_Occ``, ``_Block``, ``_ConvLayer``) read.  Shapes are free; the steps are chosen so that the
reference output of a layer is not mostly saturated:

  T = sum_K (x - zx)(w - zw) over K = cg * k * k terms.  Weight codes are uniform on 0..255 (std 73.9) and zw lies in [110, 146), so
  rms(w - zw) ~ 76 and  std(T) ~ sqrt(K) * rms(x - zx) * 76.  The weight step is set so that  sigma = std(T) * dx * mean(dw)  is the
  builder's ``sigma`` argument, the bias takes out the per-channel offset  mean(x - zx) * sum(w - zw)  (up to 18 K * mean(x - zx), which
  would otherwise pin whole channels to one end) and adds N(0.3 sigma, 0.3 sigma), and the activation step puts 3 sigma on the codes
  between a_zp and the nearer end that the output can reach (``a_delta`` ~ sqrt(K) for fixed steps).  Under ReLU about 60 % of the outputs
  are then positive and well under 1 % reach 255; without ReLU a_zp sits near the middle of the range.
"""
import numpy as np

W_RMS = 76.0            # rms of (w - zw): w uniform on 0..255, zw in [110, 146)


def uniform_stats(zx):
    """(mean, rms) of (x - zx) for codes uniform on 0..255"""
    m = 127.5 - zx
    return m, float(np.sqrt(73.9 ** 2 + m * m))


def relu_stats(zp):
    """(mean, rms) of (code - zp) of a layer built here with ReLU: code - zp = span * max(z + 0.3, 0) / 3, z ~ N(0, 1)"""
    span = 255.0 - zp
    return 0.189 * span, 0.296 * span


def act_step(sigma, a_zp, relu, mean=0.0):
    """the activation step that puts mean + 3 sigma at the end of the code range"""
    span = (255.0 - a_zp) if relu else min(a_zp, 255.0 - a_zp)
    return np.float32((abs(mean) + 3.0 * sigma) / span)


def conv_state(rng, name, cout, cg, k, in_q, in_stats, a_zp, relu=True, sigma=1.0, a_off=False):
    """One QuantModule convolution [cout, cg, k, k] on codes with quantizer ``in_q`` = (delta, zp) whose (x - zp) has ``in_stats``."""
    K = cg * k * k
    code = rng.integers(0, 256, size=(cout, cg, k, k), dtype=np.uint8)
    zw = rng.integers(110, 146, size=cout).astype(np.float32)
    dw_mean = sigma / (float(in_q[0]) * np.sqrt(K) * in_stats[1] * W_RMS)
    dw = (dw_mean * rng.uniform(0.67, 1.33, size=cout)).astype(np.float32)
    scale = np.float32(in_q[0]) * dw
    offset = in_stats[0] * (code.reshape(cout, -1).astype(np.float64) - zw[:, None]).sum(axis=1) * scale
    bias = (rng.normal(0.3 * sigma, 0.3 * sigma, size=cout) - offset).astype(np.float32)
    return {
        name + "/w_code": code, name + "/w_delta": dw, name + "/w_zp": zw, name + "/bias": bias,
        name + "/a_delta": act_step(sigma, a_zp, relu), name + "/a_zp": np.float32(a_zp), name + "/a_off": np.bool_(a_off),
    }


def conv1x1_state(rng, name, cin, cout, in_q, in_stats, a_zp, **kw):
    return conv_state(rng, name, cout, cin, 1, in_q, in_stats, a_zp, **kw)


def gconv_state(rng, name, c, cg, in_q, in_stats, a_zp, **kw):
    return conv_state(rng, name, c, cg, 3, in_q, in_stats, a_zp, **kw)


def conv3x3_state(rng, name, cin, cout, in_q, in_stats, a_zp, **kw):
    return conv_state(rng, name, cout, cin, 3, in_q, in_stats, a_zp, **kw)


def occ_state(rng, name, c, in_q, in_stats, a_zp=120):
    """the occupancy head [1, c, 1, 1]: no ReLU, a two-sided quantizer"""
    return conv_state(rng, name, 1, c, 1, in_q, in_stats, a_zp, relu=False)


def f32_variant(state, name, new_name):
    """the same layer under ``new_name`` with its activation quantizer off (``convg(..., f32_out=True)`` asserts a_off)"""
    out = {new_name + k[len(name):]: v for k, v in state.items() if k.startswith(name + "/")}
    out[new_name + "/a_off"] = np.bool_(True)
    return out


def block_quantizer(name, in_q, in_stats, sigma, a_zp):
    """``name/a_delta, a_zp`` of the quantizer after  relu(y + shortcut):  y ~ N(0.3 sigma, sigma), shortcut = (x - zx) * dx"""
    dx = float(in_q[0])
    mean = 0.3 * sigma + in_stats[0] * dx
    std = float(np.sqrt(sigma ** 2 + (in_stats[1] ** 2 - in_stats[0] ** 2) * dx * dx))
    return {name + "/a_delta": act_step(std, a_zp, True, mean), name + "/a_zp": np.float32(a_zp)}


def bottleneck_state(rng, name, planes, cg, in_q, in_stats, zp1, zp2, out_zp):
    """A whole QuantBottleneck with an identity shortcut: ``name.conv1`` (1x1, planes -> 2 planes), ``.conv2`` (grouped 3x3), ``.conv3``
    (1x1 back to planes, fp32 output) and the block quantizer.  conv3's sigma is the shortcut's spread, so both terms of the sum move codes."""
    width = 2 * planes
    s = conv1x1_state(rng, name + ".conv1", planes, width, in_q, in_stats, zp1)
    q1 = (s[name + ".conv1/a_delta"], zp1)
    s.update(gconv_state(rng, name + ".conv2", width, cg, q1, relu_stats(zp1), zp2))
    q2 = (s[name + ".conv2/a_delta"], zp2)
    sigma3 = float(np.sqrt(in_stats[1] ** 2 - in_stats[0] ** 2)) * float(in_q[0])
    s.update(conv1x1_state(rng, name + ".conv3", width, planes, q2, relu_stats(zp2), 0, sigma=sigma3, a_off=True))
    s.update(block_quantizer(name, in_q, in_stats, sigma3, out_zp))
    return s


def padded(x_u8, zp):
    """u8 [N,H,W,C] -> padded i8 [N,H+2,W+2,C] (code - 128) whose border holds the pad code ``zp`` (x - zp == 0 there)"""
    n, h, w, c = x_u8.shape
    p = np.full((n, h + 2, w + 2, c), int(zp), np.int16)
    p[:, 1:-1, 1:-1] = x_u8
    return (p - 128).astype(np.int8)
