"""Shared helpers for the parity tests (test infrastructure; may import oracle/)."""
import contextlib
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def gold(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: z[k] for k in z.files}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def make_opt(R=256, **over):
    """The `opt` fields the model reads (reference lib/opts.py:221-239, heads :291-295)."""
    o = types.SimpleNamespace(
        depth=True, heads={'hm': 2, 'wh': 2, 'params': 122}, iterations=False,
        PCA_SZ=63, knn_K=64, ball_radius=0.015, ball_radius2=0.04,
        sample_num_level1=512, sample_num_level2=128, INPUT_FEATURE_NUM=3, SAMPLE_NUM=1024,
        default_resolution=R, DECONV_DIMS=[256, 256, 256, 256], GCN_IN_DIM=[512, 256, 128],
        GCN_OUT_DIM=[256, 128, 64], IMG_DIMS=[256, 128, 64], graph_k=2, graph_layer_num=4)
    for k, v in over.items():
        setattr(o, k, v)
    return o


def surrogate_loss(res):
    """Scalar touching every model output (same definition as oracle/make_goldens.py)."""
    result, params, hand_list, other = res
    t = 0
    for h in ("left", "right"):
        t = t + result['verts3d'][h].pow(2).mean() + (result['verts2d'][h] / 384).pow(2).mean()
        t = t + params['scale'][h].pow(2).mean() + params['trans2d'][h].pow(2).mean() + params['root'][h].pow(2).mean()
        t = t + hand_list[0]['verts3d'][h].pow(2).mean()
    t = t + other['hms'].pow(2).mean() + other['mask'].pow(2).mean()
    for k in ('hm', 'wh', 'params'):
        t = t + other['ret'][k].pow(2).mean()
    return t


def pack_outputs(res, ind):
    result, params, hand_list, other = res
    o = {}
    for h in ("left", "right"):
        o["verts3d_" + h] = result['verts3d'][h]
        o["verts2d_" + h] = result['verts2d'][h]
        o["scale_" + h] = params['scale'][h]
        o["trans2d_" + h] = params['trans2d'][h]
        o["root_" + h] = params['root'][h]
        o["gcn_verts3d_" + h] = hand_list[0]['verts3d'][h]
        o["mano_list_verts3d_" + h] = other['verts3d_MANO_list'][h][0]
    B = ind.shape[0]
    p = other['ret']['params'].reshape(B, 122, -1)
    o["params_at_ind"] = torch.gather(p, 2, ind.unsqueeze(1).expand(B, 122, 2)).transpose(1, 2)
    o["hm"] = other['ret']['hm']
    o["wh_crop"] = other['ret']['wh'][:, :, 8:24, 8:24]
    for k in ("hms", "mask"):
        t = other[k]
        o[k + "_sum"] = t.double().sum().reshape(1)
        o[k + "_abs_sum"] = t.double().abs().sum().reshape(1)
        o[k + "_crop"] = t[:, :, 8:24, 8:24]
    return o


# tolerances: SURVEY.md Appendix C noise floor (fp32 vs fp64 of the oracle itself)
TOL_EVAL = {"verts3d": 1e-4, "scale": 1e-4, "trans2d": 1e-4, "root": 1e-4, "gcn_verts3d": 1e-4,
            "mano_list_verts3d": 1e-4, "params_at_ind": 1e-4, "hm": 1e-4}


def check_packed(got, exp, abs_tol=1e-4, rel_tol=1e-5, skip=()):
    """got: dict of tensors, exp: dict of numpy arrays. verts2d/hms/mask use relative tolerance."""
    bad = []
    for k, e in exp.items():
        if k not in got or k in skip:
            continue
        g = got[k].detach().cpu().double().numpy()
        e = e.astype(np.float64)
        d = np.abs(g - e).max()
        lim = abs_tol + rel_tol * np.abs(e).max()
        if k.startswith("verts2d") or k.startswith("hms") or k.startswith("mask"):
            lim = abs_tol + 5 * rel_tol * np.abs(e).max()      # pixel-scaled outputs: relative
        if not d <= lim:
            bad.append((k, d, lim))
    assert not bad, bad


def synthetic_model_outputs(B, R, seed):
    """Model-output-shaped tensors for the loss parity fixture (same generator as oracle/make_goldens.py)."""
    g = np.random.Generator(np.random.PCG64(seed))
    f = lambda *sh, sc=1.0: torch.from_numpy((g.standard_normal(sh) * sc).astype(np.float32))
    result = {'verts3d': {h: f(B, 778, 3, sc=0.05) for h in ('left', 'right')},
              'verts2d': {h: f(B, 778, 2, sc=30.0) + R / 2 for h in ('left', 'right')}}
    params = {'scale': {h: f(B, sc=0.3) for h in ('left', 'right')}, 'trans2d': {h: f(B, 2, sc=0.3) for h in ('left', 'right')},
              'root': {h: f(B, 3, sc=3.0) for h in ('left', 'right')}}
    hand = [{'verts3d': {h: f(B, 252, 3, sc=0.05) for h in ('left', 'right')},
             'verts2d': {h: f(B, 252, 2, sc=30.0) + R / 2 for h in ('left', 'right')}}]
    other = {'hms': f(B, 42, R // 4, R // 4, sc=0.3), 'mask': f(B, 2, R, R, sc=0.5),
             'ret': {'hm': f(B, 2, R // 4, R // 4) - 2.0, 'wh': f(B, 2, R // 4, R // 4), 'params': f(B, 122, R // 4, R // 4)}}
    return result, params, hand, other


def general_cameras(B, R, seed, third_row=False):
    """Per-sample camera matrices [B,3,3] float32 that are NOT the one pinhole matrix of synthetic_train_batch: K[b] = A_b @ K0 with
    K0 = [[R,0,R/2],[0,R,R/2],[0,0,1]] and A_b a 2-D affine map in homogeneous form drawn per sample -- rotation within +-30 degrees,
    scale 0.8 .. 1.2, translation within +-0.08 R (what the dataset's rotation / scale augmentation does to K): every entry of the first two
    rows is non-zero and differs between samples.  third_row=True also perturbs the last row to (e0, e1, 1 + e2), |e0|, |e1| <= 0.01,
    |e2| <= 0.02: no entry of K is then 0 or 1, and a point at depth ~0.45 still projects with a depth near 0.45."""
    g = np.random.Generator(np.random.PCG64(seed))
    ang = g.uniform(-np.pi / 6, np.pi / 6, B)
    s = g.uniform(0.8, 1.2, B)
    t = g.uniform(-0.08 * R, 0.08 * R, (B, 2))
    e = g.uniform(-1.0, 1.0, (B, 3)) * np.array([0.01, 0.01, 0.02])
    A = np.zeros((B, 3, 3))
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = s * np.cos(ang), -s * np.sin(ang), t[:, 0]
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = s * np.sin(ang), s * np.cos(ang), t[:, 1]
    A[:, 2, 2] = 1.0
    K = A @ np.array([[R, 0, R / 2], [0, R, R / 2], [0, 0, 1]], np.float64)
    if third_row:
        K[:, 2] = e + np.array([0.0, 0.0, 1.0])
    K = K.astype(np.float32)
    for b in range(1, B):
        assert (np.abs(K[b, :2] - K[:b, :2]).min(axis=0) > 0).all()      # every sample's entries are its own
    assert (K[:, :2] != 0).all()
    return torch.from_numpy(K)


def aten_dense_terms(mask, mask_gt, hms, hms_gt, hm, hm_gt):
    """The dense-map terms of the reference with aten ops (checker; any float dtype): SmoothL1 on the masks, MSE on the joint heat-maps,
    CornerNet focal loss [B] on the clamped sigmoid of the centre map (simplified.py:368,374,376,391; losses.py:138-165)."""
    import torch.nn.functional as TF
    p = torch.clamp(torch.sigmoid(hm), 1e-4, 1 - 1e-4)
    pos, neg = hm_gt.eq(1).to(hm.dtype), hm_gt.lt(1).to(hm.dtype)
    pl = (torch.log(p) * (1 - p) ** 2 * pos).sum((1, 2, 3))
    nl = (torch.log(1 - p) * p ** 2 * (1 - hm_gt) ** 4 * neg).sum((1, 2, 3))
    npos = pos.sum((1, 2, 3))
    focal = -nl if float(npos.sum()) == 0 else -(pl + nl) / (npos + 1e-3)
    return TF.smooth_l1_loss(mask, mask_gt), TF.mse_loss(hms, hms_gt), focal


def face_terms_ref(p, q, fc):
    """(normal loss, edge-length loss) of lib/trains/simplified.py:66-115 for ONE hand with aten ops (checker; any float dtype):
    p, q [B,V,3] prediction / ground truth, fc [F,3] int64."""
    import torch.nn.functional as TF
    unit = lambda v: TF.normalize(v, p=2, dim=2)
    f0, f1, f2 = fc[:, 0], fc[:, 1], fc[:, 2]
    n = unit(torch.cross(unit(q[:, f1] - q[:, f0]), unit(q[:, f2] - q[:, f0]), dim=2))
    cos = [torch.abs((unit(v) * n).sum(2, keepdim=True)) for v in (p[:, f1] - p[:, f0], p[:, f2] - p[:, f0], p[:, f2] - p[:, f1])]
    d = lambda x, i, j: torch.sqrt(((x[:, i] - x[:, j]) ** 2).sum(2, keepdim=True))
    ed = [torch.abs(d(p, i, j) - d(q, i, j)) for i, j in ((f0, f1), (f0, f2), (f1, f2))]
    return torch.cat(cos, 1).mean(), torch.cat(ed, 1).mean()


def tree_to(obj, device):
    if torch.is_tensor(obj):
        return obj.to(device)
    if isinstance(obj, dict):
        return {k: tree_to(v, device) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(tree_to(v, device) for v in obj)
    return obj


def demo_fixture_inputs(device='cpu'):
    """BASELINE config 1: the network input of the reference's demo (demo.py:117-202) rebuilt from
    tests/golden/demo_H2O_000002_R256.npz -- uint8 BGR image -> ImageNet-normalised NCHW, uint16 millimetres -> metres --
    plus the clouds the reference's own depth2pcl produced.  -> (golden dict, batch dict)."""
    g = gold("demo_H2O_000002_R256")
    mean = np.array([0.485, 0.456, 0.406], np.float32).reshape(1, 1, 3)
    std = np.array([0.229, 0.224, 0.225], np.float32).reshape(1, 1, 3)
    pre = ((g["image_u8"].astype(np.float32) / 255. - mean) / std).astype(np.float32)
    b = {'input': torch.from_numpy(pre).permute(2, 0, 1).unsqueeze(0).contiguous(),
         'depth': torch.from_numpy(g["depth_mm_u16"].astype(np.float32) / 1000.).reshape(1, 1, 256, 256),
         'K_new': torch.from_numpy(g["K_img"].astype(np.float32)).reshape(1, 3, 3),
         'valid': torch.ones(1, 2), 'choose': torch.from_numpy(g["choose"]).unsqueeze(0), 'cloud': torch.from_numpy(g["cloud"]).unsqueeze(0)}
    return g, {k: v.to(device) for k, v in b.items()}


def demo_state_dict(template, g):
    """Generator weights + the mask-head bias shift the fixture was made with (oracle/make_demo_golden.py)."""
    from oracle import synth
    sd = synth.det_state_dict(template)
    sd['encoder.dp_decoder.final_layer.1.bias'] = sd['encoder.dp_decoder.final_layer.1.bias'] + torch.from_numpy(g["dp_bias_add"])
    return sd


def pack_demo(res):
    result, params, hand, other = res
    o = {}
    for h in ("left", "right"):
        o["verts3d_" + h] = result['verts3d'][h]
        o["verts2d_" + h] = result['verts2d'][h]
        o["scale_" + h] = params['scale'][h]
        o["trans2d_" + h] = params['trans2d'][h]
        o["root_" + h] = params['root'][h]
        o["gcn_verts3d_" + h] = hand[0]['verts3d'][h]
    o["hm"] = other['ret']['hm']
    for k in ("hms", "mask"):
        t = other[k]
        o[k + "_sum"] = t.double().sum().reshape(1)
        o[k + "_abs_sum"] = t.double().abs().sum().reshape(1)
        o[k + "_crop"] = t[:, :, 8:24, 8:24]
    return o


def build_c_client(out_dir):
    """Compile tests/c_abi/c_client.c (plain C, gcc) against include/pdfnet_hip.h and libpdfnet_hip.so -> path of the binary."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "pdfnet_amd")
    exe = os.path.join(str(out_dir), "c_client")
    cmd = ["gcc", "-O1", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(root, "tests", "c_abi", "c_client.c"), "-o", exe, "-L", lib, "-lpdfnet_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


# ----------------------------------------------------------------------------------------------
# Dropout: pin the seed a site draws, and recover the keep-mask a kernel used from the kernel itself (tests/test_dropout_gpu.py).
# The masks are counter-based -- a pure function of (host seed, device step counter, element index) -- so a probe with the same seed and
# step on inputs made of zeros and ones reads the mask back without restating the hash.
@contextlib.contextmanager
def pinned_seeds(F, seeds, step=0):
    """While active, F.next_seed() hands out `seeds` in order (every dropout site calls the module-level function) and the device step
    counter holds `step`.  -> namespace with .seeds and .drawn (how many were taken; one more than there are is an error).
    F._seed_state[0], the step counter's value and F.next_seed itself are put back on exit."""
    counter = F.step_counter(torch.device('cuda', torch.cuda.current_device()))
    saved_state, saved_step, saved_fn = F._seed_state[0], int(counter.item()), F.next_seed
    pin = types.SimpleNamespace(seeds=[int(s) for s in seeds], drawn=0)

    def draw():
        assert pin.drawn < len(pin.seeds), "a dropout site drew seed number %d of %d pinned ones" % (pin.drawn + 1, len(pin.seeds))
        pin.drawn += 1
        return pin.seeds[pin.drawn - 1]
    F.next_seed = draw
    counter.fill_(int(step))
    try:
        yield pin
    finally:
        torch.cuda.synchronize()
        F.next_seed = saved_fn
        F._seed_state[0] = saved_state
        counter.fill_(saved_step)


@contextlib.contextmanager
def recorded_seeds(F):
    """While active, every seed F.next_seed() hands out is appended to the list this yields (the seeds themselves are unchanged)."""
    saved_fn, log = F.next_seed, []

    def draw():
        log.append(saved_fn())
        return log[-1]
    F.next_seed = draw
    try:
        yield log
    finally:
        F.next_seed = saved_fn


def probe_dropout_mask(F, shape, p, seed, step=0):
    """Keep-mask of F.dropout at `shape` (bool, CPU): dropout(ones) > 0."""
    with pinned_seeds(F, [seed], step):
        y = F.dropout(torch.ones(shape, device='cuda'), p, True)
        return (y > 0).cpu()


def probe_dropout_add_mask(F, shape, p, seed, step=0):
    """Keep-mask of F.dropout_add at `shape`: dropout_add(ones, zeros) > 0."""
    with pinned_seeds(F, [seed], step):
        y = F.dropout_add(torch.ones(shape, device='cuda'), torch.zeros(shape, device='cuda'), p, True)
        return (y > 0).cpu()


def probe_ln_fused_mask(F, shape, p, seed, step=0):
    """Keep-mask of the fused-LayerNorm site on x [2, ..., Fd] with paired parameters: x = 0 is the residual, add = 1 the dropped operand,
    so the returned residual stream z is mask / (1 - p)."""
    Fd = shape[-1]
    one, zero = torch.ones(Fd, device='cuda'), torch.zeros(Fd, device='cuda')
    with pinned_seeds(F, [seed], step):
        z, _ = F.layer_norm_fused(torch.zeros(shape, device='cuda'), one, zero, 1e-6, F.ACT_NONE, add=torch.ones(shape, device='cuda'), p=p,
                                  training=True, gamma1=one, beta1=zero)
        return (z > 0).cpu()


def probe_attention_mask(F, nb, V, Fd, heads, p, seed, step=0, kv_shift=0):
    """Keep-mask of F.attention's probabilities, [nb, heads, V (query), V (key)] bool on the CPU.  q = k = 0 makes every probability 1 / V;
    v[b, j, h * dh + c] = 1 iff j == base + c turns output feature c of head h into (mask of key base + c) / ((1 - p) V); base walks over
    the keys in ceil(V / dh) calls with the same seed."""
    dh = Fd // heads
    q = torch.zeros(nb, V, Fd, device='cuda')
    mask = torch.zeros(nb, heads, V, V, dtype=torch.bool)
    calls = (V + dh - 1) // dh
    with pinned_seeds(F, [seed] * calls, step) as pin:
        for base in range(0, V, dh):
            n = min(dh, V - base)
            v = torch.zeros(nb, V, heads, dh)
            for c in range(n):
                v[:, base + c, :, c] = 1
            out = F.attention(q, q, v.reshape(nb, V, Fd).cuda(), heads, p, True, kv_shift)
            mask[:, :, :, base:base + n] = (out.reshape(nb, V, heads, dh)[..., :n] > 0).permute(0, 2, 1, 3).cpu()
        assert pin.drawn == calls
    return mask


# ----------------------------------------------------------------------------------------------
# Which kernels ran: the library's per-kernel records (pdf_debug_kernel_timing / _record; the names are the strings the sources give to
# KTimer).  tests/test_gemm_dispatch_gpu.py pins the kernel every parity case is meant for with it.
@contextlib.contextmanager
def kernels_run(F):
    """Yields a list that, on leaving the block, holds the recorded kernel symbol of every GEMM-family launch issued inside it, in launch
    order (deferred weight gradients are flushed and the device is idle before the records are read).  Recording is switched off on exit,
    also when the block raises.  The Winograd transforms carry no record: whether a launch took the Winograd path is what
    pdf_conv2d_winograd_workspace_floats says about it."""
    import ctypes
    L = F._L()
    names = []
    assert L.pdf_debug_kernel_timing(1) == 0
    try:
        yield names
        F.join_wgrad()
        torch.cuda.synchronize()
        nm = ctypes.create_string_buffer(128)
        fl, by, ms = ctypes.c_double(), ctypes.c_double(), ctypes.c_float()
        for i in range(L.pdf_debug_kernel_record_count()):
            assert L.pdf_debug_kernel_record(i, nm, 128, ctypes.byref(fl), ctypes.byref(by), ctypes.byref(ms)) == 0
            names.append(nm.value.decode())
    finally:
        L.pdf_debug_kernel_timing(0)


# ----------------------------------------------------------------------------------------------
def adam_float64(p0, grads, corrs, lr, b1, b2, eps, grad_scale=1.0):
    """Textbook Adam in float64 on exactly the float32 inputs a sequence of pdf_adam_step calls sees: lr, b1, b2, eps and grad_scale rounded to
    float32 (1 - b1 and 1 - b2 are then exact in both precisions), grads[t] the float32 gradient of call t and corrs[t] its float32
    [1 - b1^t, 1 - b2^t] exactly as uploaded.  m and v start at 0.  -> (p, m, v) in float64."""
    lr, b1, b2, eps, grad_scale = (float(np.float32(a)) for a in (lr, b1, b2, eps, grad_scale))
    p = p0.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for g, c in zip(grads, corrs):
        assert g.dtype == torch.float32 and c.dtype == torch.float32
        g = g.double() * grad_scale
        bc1, bc2 = c.double().tolist()
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return p, m, v
