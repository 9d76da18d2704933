"""Scene editing in stock torch, written from the formulas of include/egr_raytracer.h (egr_edit_select / egr_edit_apply), not from the kernel and not from
the reference's text: the selection of the objects and the eight edited arrays, parametrised by dtype and device (fp32 on the device: the operation-for-operation
peer of the kernel and of the torch sequence the fused pass replaces; fp64 on the CPU: the yardstick both are measured against).

The constants of an edit (rotation matrix, quaternion, log(scale), pi * hue_shift, override^2, the centre) are computed here in fp64 on their own path -
the matrix comes from the quaternion, not from Rodrigues' formula as in editing.py - and then cast to the dtype."""
import math

import numpy as np
import torch

ATTRS = ("_scaling", "_rotation", "_xyz", "_opacity", "_diffuse", "_normal", "_roughness", "_f0")  # the export order
TWO_PI, SECTOR = 2.0 * math.pi, math.pi / 3.0
RANGES = ("f0", "roughness", "diffuse")


def as_params(pc, dtype, device):
    """dict raw attribute -> tensor of `dtype` on `device` (fp32 -> fp64 is exact)."""
    return {a: getattr(pc, a).detach().to(device=device, dtype=dtype) for a in ATTRS}


def _bounds(box, dtype, device):
    f32 = lambda v: torch.tensor(np.asarray(v, np.float32), device=device).to(dtype)  # the bounds ARE fp32 numbers
    return f32(box["min"]), f32(box["max"])


def _inside(p, lo, hi):
    return ((p >= lo) & (p <= hi)).all(dim=1)


def shape_mask(p, box, dtype, device):
    lo, hi = _bounds(box, dtype, device)
    if "cyl" in box:
        c, h = 0.5 * (lo[:2] + hi[:2]), 0.5 * (hi[:2] - lo[:2])
        return ((((p[:, :2] - c) / h) ** 2).sum(dim=1) <= 1.0) & (p[:, 2] >= lo[2]) & (p[:, 2] <= hi[2])
    return _inside(p, lo, hi)


def select(params, boxes):
    """dict name -> bool [N]: the rows of every object of `boxes`, on the unedited raw parameters of `params` (a dict of as_params)."""
    p = params["_xyz"]
    dtype, device = p.dtype, p.device
    out = {}
    for name, box in boxes.items():
        if name == "everything":
            out[name] = torch.ones(p.shape[0], dtype=torch.bool, device=device)
            continue
        sel = shape_mask(p, box, dtype, device)
        lo, hi = _bounds(box, dtype, device)
        exempt = torch.zeros_like(sel)
        if "zrange" in box:
            exempt = _inside(p, lo + (hi - lo) * torch.tensor(np.asarray(box["zrange"], np.float32), device=device).to(dtype), hi)
        for prop in RANGES:
            if prop in box:
                x = params["_" + prop]
                mean = x.sum(dim=1) / x.shape[1]
                sel = sel & (((mean >= float(np.float32(box[prop][0]))) & (mean <= float(np.float32(box[prop][1])))) | exempt)
        for other in box.get("exclude", ()):
            sel = sel & ~shape_mask(p, boxes[other], dtype, device)
        out[name] = sel
    return out


def mask_bits(selections, names):
    """int32 [N]: bit k = selections[names[k]] (the layout of the kernel's mask; bit 31 is the sign bit)."""
    m = torch.zeros_like(next(iter(selections.values())), dtype=torch.int64)
    for k, name in enumerate(names):
        m |= selections[name].to(torch.int64) << k
    return torch.where(m >= 2 ** 31, m - 2 ** 32, m).to(torch.int32)


def rotation_constants(rx, ry, rz):
    """(R, q) in fp64 of the rotation by the axis-angle vector deg2rad(rx, ry, rz): the unit quaternion first, the matrix from it."""
    v = np.array([rx, ry, rz], np.float64) * (math.pi / 180.0)
    theta = math.sqrt(float(v @ v))
    if theta == 0.0:
        return np.eye(3), np.array([1.0, 0.0, 0.0, 0.0])
    w, (x, y, z) = math.cos(theta / 2.0), math.sin(theta / 2.0) * v / theta
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R, np.array([w, x, y, z])


def _colour(x, override, hue_shift, s_shift, s_mult, v_shift, v_mult):
    dtype, device = x.dtype, x.device
    x = torch.lerp(x, torch.tensor(override[:3], dtype=dtype, device=device).expand_as(x), float(override[3]))
    r, g, b = x.unbind(dim=1)
    mx, mn = torch.maximum(r, torch.maximum(g, b)), torch.minimum(r, torch.minimum(g, b))
    d = mx - mn
    s, v = d / (mx + 1e-8), mx
    dd = torch.where(d == 0, torch.ones_like(d), d)
    h6 = torch.where(r == mx, (g - b) / dd, torch.where(g == mx, 2.0 + (b - r) / dd, 4.0 + (r - g) / dd))
    h6 = torch.where(h6 < 0, h6 + 6.0, h6)
    h = torch.where(d == 0, torch.zeros_like(d), h6 * SECTOR)
    h = h + math.pi * hue_shift
    h = h - TWO_PI * torch.floor(h / TWO_PI)
    h = torch.where(h < 0, h + TWO_PI, h)
    h = torch.where(h >= TWO_PI, h - TWO_PI, h)
    s = (s_mult * (s + s_shift)).clamp(0.0, 1.0)
    v = (v_mult * (v + v_shift)).clamp(min=0.0)
    h6 = h / SECTOR
    fl = torch.floor(h6)
    f = h6 - fl
    hi = fl.long() % 6
    p, q, t = v * (1.0 - s), v * (1.0 - f * s), v * (1.0 - (1.0 - f) * s)
    table = torch.stack([torch.stack(c, dim=1) for c in ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))])  # [6, N, 3]
    return table.gather(0, hi[None, :, None].expand(1, -1, 3))[0]


def _colour_is_default(override, hue_shift, s_shift, s_mult, v_shift, v_mult):
    return override[3] == 0 and hue_shift == 0 and s_shift == 0 and s_mult == 1 and v_shift == 0 and v_mult == 1


def _rotate(x, R):
    return (x[:, None, :] * R[None, :, :]).sum(dim=2)  # row i: R x_i (elementwise: no matmul library in the way)


def edited(params, selections, names, edits, boxes):
    """dict raw attribute -> edited tensor: every edit of `names`, in that order, each on the result of the one before it, on its object's rows. A group
    of an edit whose fields are at their defaults is skipped."""
    out = {a: t.clone() for a, t in params.items()}
    dtype, device = out["_xyz"].dtype, out["_xyz"].device
    const = lambda v: torch.tensor(np.asarray(v, np.float64), device=device).to(dtype)
    for name in names:
        e, sel = edits[name], selections[name]
        rows = sel[:, None]
        if e.use_roughness_override or e.roughness_shift != 0 or e.roughness_mult != 1:
            r = out["_roughness"]
            base = torch.full_like(r, float(e.roughness_override) ** 2) if e.use_roughness_override else r
            out["_roughness"] = torch.where(rows, (e.roughness_mult * (base + abs(e.roughness_shift))).clamp(0.0, 1.0), r)
        dif = (e.diffuse_override, e.diffuse_hue_shift, e.diffuse_saturation_shift, e.diffuse_saturation_mult, e.diffuse_value_shift, e.diffuse_value_mult)
        if not _colour_is_default(*dif):
            out["_diffuse"] = torch.where(rows, _colour(out["_diffuse"], *dif), out["_diffuse"])
        spe = (e.specular_override, e.specular_hue_shift, e.specular_saturation_shift, e.specular_saturation_mult, e.specular_value_shift, e.specular_value_mult)
        if not _colour_is_default(*spe):
            out["_f0"] = torch.where(rows, _colour(out["_f0"], *spe), out["_f0"])
        if (e.translate_x, e.translate_y, e.translate_z, e.rotate_x, e.rotate_y, e.rotate_z) != (0,) * 6 or e.scale != 1:
            t64 = np.array([e.translate_x, e.translate_y, e.translate_z], np.float64)
            box = boxes[name]
            t, c = const(t64), const(0.5 * (np.asarray(box["min"], np.float64) + np.asarray(box["max"], np.float64)) + t64)
            R64, q64 = rotation_constants(e.rotate_x, e.rotate_y, e.rotate_z)
            R, qr = const(R64), const(q64)
            host = np.float32 if dtype == torch.float32 else np.float64  # the two scalars in the array's precision, computed on the host
            scale, log_scale = float(host(e.scale)), float(host(math.log(e.scale)))
            p = out["_xyz"] + t
            p = (p - c) * scale + c
            p = _rotate(p - c, R) + c
            out["_xyz"] = torch.where(rows, p, out["_xyz"])
            out["_normal"] = torch.where(rows, _rotate(out["_normal"], R), out["_normal"])
            out["_scaling"] = torch.where(rows, out["_scaling"] + log_scale, out["_scaling"])
            q = out["_rotation"]
            w, x, y, z = (q / torch.sqrt((q * q).sum(dim=1, keepdim=True))).unbind(dim=1)
            prod = torch.stack([qr[0] * w - qr[1] * x - qr[2] * y - qr[3] * z, qr[0] * x + qr[1] * w + qr[2] * z - qr[3] * y,
                                qr[0] * y - qr[1] * z + qr[2] * w + qr[3] * x, qr[0] * z + qr[1] * y - qr[2] * x + qr[3] * w], dim=1)
            out["_rotation"] = torch.where(rows, prod, q)
        if e.removed:
            out["_opacity"] = torch.where(rows, torch.full_like(out["_opacity"], -1e8), out["_opacity"])
    return out


def rotation_matrices(q):
    """[N,3,3] fp64 rotation matrices of the normalised quaternions q [N,4] (w, x, y, z): what the tracer sees of a rotation (the sign of q drops out)."""
    q = q.detach().to("cpu", torch.float64)
    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(dim=1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
