"""NumPy float32 restatement of the SGD-momentum step of csrc/k_optim.h (rd_sgd_mom_update): one rounding per operation, in the order the
header states, no fused multiply-add (NumPy's float32 array arithmetic rounds every product and sum on its own).  The weight images come
from the library's own host packers applied to the model's updated weights."""
import numpy as np

F32 = np.float32


def sgd_step(w, g, m, lr, momentum, wd, rescale_grad, clip_gradient, lr_mult=1.0, wd_mult=1.0):
    """float32 arrays w, g, m of one shape -> (new w, new m).  The scalars are rounded to float32 first (the C ABI takes floats)."""
    w, g, m = (np.asarray(v, F32) for v in (w, g, m))
    lr_t = F32(lr) * F32(lr_mult)
    wd_t = F32(wd) * F32(wd_mult)
    lrwd = F32(lr_t * wd_t)
    g = F32(rescale_grad) * g
    if clip_gradient >= 0:
        c = F32(clip_gradient)
        g = np.where(g > c, c, np.where(g < -c, -c, g)).astype(F32)     # a NaN fails both comparisons and stays
    a = F32(momentum) * m
    b = lrwd * w
    c2 = lr_t * g
    m2 = ((a - b) - c2).astype(F32)
    return (w + m2).astype(F32), m2


def flip_weight(w):
    """the weight of the data gradient: channel axes swapped, taps flipped"""
    return np.ascontiguousarray(np.asarray(w, F32).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def forward_image(L, w, fold_scale, dt):
    """bytes of rd_pack_conv3x3_ex_host(w, fold_scale, cout, cin, 1, cin, dt)"""
    return L.pack_conv3x3_ex(np.asarray(w, F32), 1, w.shape[1], fold_scale=fold_scale, dtype=dt)


def data_grad_image(L, w, dt):
    """TowerOps.pack_data_grad's image"""
    return L.pack_conv3x3_ex(flip_weight(w), 1, w.shape[0], fold_scale=None, dtype=dt)


def tie_values(shape, dt, rng, bf16):
    """float32 values exactly halfway between two neighbours of the 16-bit type, magnitudes in 1/8 .. 2, both parities of the last kept bit"""
    n = int(np.prod(shape))
    keep = 16 if bf16 else 13                                    # float32 mantissa bits the type drops
    v = (rng.uniform(0.125, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    u = v.view(np.uint32)
    u = (u >> keep << keep) | np.uint32(1 << (keep - 1))
    out = u.astype(np.uint32).view(F32).reshape(shape)
    last = (u >> keep) & 1
    assert 0.3 < last.mean() < 0.7                               # ties to an even and to an odd neighbour both occur
    return out
