"""The conv launches the suite pins against the recorded decisions of the commit before the conv
route became one host-only module (tests/golden/conv_routes.json), shared by
test_conv_route_cpu.py (every row, no launch) and test_kernels_gpu.py (the GEMM / patch cases,
which assert their route before they launch).

A row is one launch as the kernel sees it: the kernel, its template parameters (t.*), grid,
block, dynamic LDS bytes and every scalar of its args struct (a.*), keyed as the recording
binding wrote them.
"""

import hashlib
import json

import numpy as np

import conv_forms
from gale.models.graph import conv_n_tiles, round_up

BATCHES = (1, 2, 3, 5, 8, 16, 32, 64, 100, 128, 256, 1024)
POLICIES = ((0, 1), (1, 1), (2, 1), (0, 0), (0, 2))  # (set_conv_path, set_conv_patch)
FULL_ROWS = (1, 64, 256)  # batches whose rows the golden file keeps in full, policy (0, 1)
KERNELS = ("none", "f32", "gemm", "patch", "mfma")

GEMM_CASES = [
    # B, H, W, Cin, Cout, k, stride, pad, residual
    (2, 14, 14, 64, 64, 3, 1, 1, False),      # ResNet-50 stage 1 3x3 (BN = 64), M % 128 != 0
    (3, 9, 11, 64, 128, 3, 2, 1, True),       # strided 3x3, odd sizes, BN = 128, residual
    (2, 14, 14, 256, 128, 1, 2, 0, False),    # 1x1 stride-2 projection
    (4, 7, 7, 128, 512, 1, 1, 0, True),       # 1x1 expand + residual
    (1, 7, 7, 512, 512, 3, 1, 1, False),      # K = 4608 (72 k-steps)
    (3, 7, 9, 64, 256, 1, 1, 0, False),       # K = 64: the single-stage form, BN = 64 of Npad 256
]
# (bn, stages) of conv_gemm's launch for each case
GEMM_FORMS = [(64, 2), (128, 2), (128, 2), (128, 2), (128, 2), (64, 1)]

PATCH_CASES = [  # B, H, W, Cin, Cout, with_res: the ResNet-50 3x3 stride-1 shapes (+ residual)
    (2, 56, 56, 64, 64, False),     # 2 rows x 56 per tile, BN = 64, 240-row patch
    (3, 28, 28, 128, 128, True),    # 4 rows x 28, BN = 128
    (2, 14, 14, 256, 256, False),   # 7 rows x 14 (98 of 128 MFMA rows), two channel tiles
    (1, 14, 14, 128, 64, True),     # BN = 64 at 14 x 14
    (3, 7, 7, 512, 512, True),      # two whole 7 x 7 images per tile, a partial last tile
]
# (bn, prr) of conv_patch's launch for each case under set_conv_patch(2)
PATCH_FORMS = [(64, 240), (128, 184), (128, 152), (64, 152), (128, 184)]

TAP_CASES = [(56, 64, 4), (28, 128, 0), (14, 256, 8), (28, 128, 5), (7, 128, 0), (7, 128, 8)]


def conv_desc(H, W, Cin, Cout, k, stride, pad, res=False, relu=True):
    """The ConvDesc dict ops.pack_conv + ops.conv2d make for a bf16 launch (identity residual)."""
    cout = round_up(Cout, 4)
    K = k * k * Cin
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    d = dict(Cin=Cin, Cout=cout, KH=k, KW=k, K=K, Kpad=round_up(K, 32),
             Npad=round_up(cout, conv_n_tiles(cout) * 16), H=H, W=W, Ho=Ho, Wo=Wo, stride=stride,
             pad=pad, relu=int(relu), in_f32=0, out_f32=0)
    if res:
        d.update(has_res=1, res_H=Ho, res_W=Wo, res_C=cout, res_stride=1)
    return d


def gemm_desc(case):
    _, H, W, Cin, Cout, k, s, p, res = case
    return conv_desc(H, W, Cin, Cout, k, s, p, res)


def patch_desc(case):
    _, H, W, Cin, Cout, res = case
    return conv_desc(H, W, Cin, Cout, 3, 1, 1, res)


def suite_descs():
    """[(source, desc, has_res)] of the kernel tests: conv_forms.py and the GEMM / patch cases."""
    out = []
    for f in conv_forms.FORMS:
        for fp8 in (False, True):
            out.append((f"form:{f.name}:{'fp8' if fp8 else 'bf16'}", conv_forms.desc(f, fp8),
                        f.res is not None))
    for c in GEMM_CASES:
        out.append((f"gemm:{c}", gemm_desc(c), c[-1]))
    for c in PATCH_CASES:
        out.append((f"patch:{c}", patch_desc(c), c[-1]))
    for H, C, _ in TAP_CASES:
        out.append((f"tap:{H}x{C}", conv_desc(H, H, C, C, 3, 1, 1, relu=False), False))
    return out


def plan_descs(name, ops):
    """[(source, desc, has_res)] of a zoo plan's conv and conv_proj ops."""
    return [(f"{name}:{i}", op["conv"], bool(op["res"] >= 0 and op["conv"]["has_res"]))
            for i, op in enumerate(ops) if op["kind"] in (0, 11)]


def distinct(entries):
    """{key: (desc, has_res, [sources])} in first-seen order; the key is the canonical JSON."""
    out = {}
    for src, d, has_res in entries:
        key = json.dumps([d, bool(has_res)], sort_keys=True)
        out.setdefault(key, (d, bool(has_res), []))[2].append(src)
    return out


def _f32(v):
    return float(np.float32(v))


def row_of_route(d, batch, has_res, r):
    """The launch row of conv_route()'s dict `r` for desc dict `d`: the args struct as the launcher
    fills it from the desc and the plan."""
    g = lambda k, dflt=0: d.get(k, dflt)
    kernel = KERNELS.index(r["kernel"])
    if kernel == 0:
        return {"kernel": 0}
    row = {"kernel": kernel, "block": 256, "lds": 0, "grid_y": 1, "a.has_res": int(has_res),
           "a.relu": g("relu"), "a.H": d["H"], "a.W": d["W"], "a.Cin": d["Cin"],
           "a.Cout": d["Cout"], "a.Kpad": d["Kpad"]}
    res = {"a.res_H": g("res_H", d["Ho"]), "a.res_W": g("res_W", d["Wo"]),
           "a.res_C": g("res_C", d["Cout"]), "a.res_stride": g("res_stride", 1)}
    conv = {"a.M": r.get("M"), "a.HWo": d["Ho"] * d["Wo"], "a.Wo": d["Wo"], "a.KW": d["KW"],
            "a.stride": d["stride"], "a.pad": d["pad"]}
    if r["kernel"] == "f32":
        row.update(conv, **res)
        row.update({"grid_x": r["grid_m"], "grid_y": r["grid_n"], "a.Ho": d["Ho"], "a.K": d["K"],
                    "a.Npad": d["Npad"]})
    elif r["kernel"] == "gemm":
        row.update(conv)
        row.update({"grid_x": r["nwg"], "t.BM": 128, "t.BN": r["bn"], "t.STEM": r["stem"],
                    "t.NST": r["stages"], "a.nkb": r["nkb"], "a.nkb1": r["nkb"],
                    "a.cin_blocks": r["cin_blocks"], "a.out_f32": g("out_f32"),
                    "a.n_tiles": r["n_tiles"], "a.nwg": r["nwg"]})
    elif r["kernel"] == "patch":
        row.update({"grid_x": r["nwg"], "t.BN": r["bn"], "t.PRR": r["prr"], "a.B": r["batch"],
                    "a.n_tiles": r["n_tiles"], "a.nwg": r["nwg"]})
        row.update({f"a.{k}": r[k] for k in ("TR", "P", "PW", "PR", "rblocks", "IMG", "PR1",
                                             "nsteps")})
    else:
        f8 = bool(g("fp8"))
        mode = ("fast", "gather", "1x1").index(r["mode"])
        row.update(conv, **res)
        row.update({"grid_x": r["grid_m"], "grid_y": r["n_blocks"], "lds": r["lds_bytes"],
                    "t.NT": r["nt"], "t.PR": r["pr"], "t.MODE": mode, "t.IN_F32": g("in_f32"),
                    "t.OUT_F32": g("out_f32") if mode == 2 else 0, "t.F8": int(f8),
                    "a.Ho": d["Ho"], "a.K": d["K"], "a.cin_shift": r["cin_shift"],
                    "a.kw_magic": r["kw_magic"], "a.BK": r["bk"], "a.nkc": r["nkc"],
                    "a.m_tiles": r["m_tiles"],
                    "a.in_scale": _f32(g("in_scale", 1.0)) if f8 else 1.0,
                    "a.in_qinv": float(np.float32(1) / np.float32(g("in_scale", 1.0))) if f8 else 1.0,
                    "a.out_qinv": float(np.float32(1) / np.float32(g("out_scale", 1.0))) if f8 else 1.0,
                    "a.res_scale": _f32(g("res_scale", 1.0)) if f8 else 1.0})
    return row


def canon(row):
    """Integral values as ints (the recording binding wrote doubles)."""
    return {k: int(v) if float(v).is_integer() else float(v) for k, v in row.items()}


def digest(rows):
    """sha256[:16] over the sorted [path, patch, batch, row] records of one desc."""
    text = json.dumps(sorted(rows, key=lambda r: r[:3]), sort_keys=True)
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def key_digest(key):
    """sha256[:16] of a distinct() key: the golden file names a desc by it."""
    return hashlib.sha256(key.encode()).hexdigest()[:16]


# The scalars a launcher copies from the desc unchanged. The golden file's per-desc hash covers
# them; its full rows leave them out and keep what the route decides.
DESC_COPIES = {"a." + k for k in ("H", "W", "Cin", "Ho", "Wo", "HWo", "Cout", "KW", "stride", "pad",
                                  "K", "Kpad", "Npad", "relu", "out_f32", "res_H", "res_W", "res_C",
                                  "res_stride", "in_scale", "in_qinv", "out_qinv", "res_scale")}


def decided(row):
    """[[key, value], ...] of a row without the desc copies, sorted by key."""
    return [[k, row[k]] for k in sorted(row) if k not in DESC_COPIES]


def form_of(row):
    """(kernel name, template parameters) of a row."""
    return (KERNELS[row["kernel"]],) + tuple((k[2:], row[k]) for k in sorted(row) if k[:2] == "t.")
