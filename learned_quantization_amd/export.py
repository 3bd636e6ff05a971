"""Integer export + compression (SURVEY f-1): the reference's end-of-run artefact.

Mirrors ``save_compress_parameters`` of
/root/reference/CIFAR-10/nested_quantization_layer/utils/log_scripts.py:61-97:

    weights[layer.name + '/W'] = floor(kernel / scale).astype(int8)      (:74-76)
    weights[layer.name + '/b'] = floor(b / b_scale).astype(int8)         (:77-79)
    np.save(log_dir/weights.npy, weights)  -> zip(ZIP_DEFLATED) -> file_sizes.log in MB  (:83-97)

The integers come from the HIP kernel K1 (``q_dtype = int8``: the same two's-complement wrap as
``astype(np.int8)``; the reference's cast silently wraps when |q| > 127, e.g. at the initial scale).
Layouts are the reference's (HWIO / (in,out)), so the arrays are byte-compatible.  Plain (non-custom)
conv/dense layers are stored in float32 like the reference does for "conv2d" layers (:80-82).
The reference does not store the scales (thesis chapter4.tex:328-330 notes they must be kept separately);
``scales.npz`` is written next to the archive as an extension.
"""
from __future__ import annotations

import json
import math
import os
import zipfile
from typing import Dict, List

import numpy as np
import torch

from . import ops
from .descriptor import group_geometry, init_geometry
from .layers import CustomQuantizedScaleLayer, quantized_tensors      # the one walk both exports use


def _host(t: torch.Tensor) -> np.ndarray:
    """C-contiguous host array in the tensor's LOGICAL index order.  A conv kernel stored in OIHW order behind its HWIO shape comes
    back from ``.cpu().numpy()`` with permuted strides -- a 1x1 kernel even F-contiguous, which numpy pickles in Fortran byte order:
    the bytes of weights.npy (and the compressed size in file_sizes.log) would then depend on the storage."""
    return np.ascontiguousarray(t.detach().cpu().numpy())


def quantized_state(model: torch.nn.Module) -> Dict[str, np.ndarray]:
    # a layer with an integer range exports the CLAMPED integers (nested.quantized_integers): inside the range whatever
    # floor(P/s) is, so int8 cannot wrap for bits <= 8 (rint(P/s) for a rounding="nearest" layer: the view is the layer's own); a
    # layer without one exports floor(P/s) as before
    return {name: _host(nested.quantized_integers(param.data, torch.int8))
            for name, param, nested in quantized_tensors(model)}


def _pack_source(param: torch.nn.Parameter, nested: CustomQuantizedScaleLayer):
    """(P, s) whose floor(P/s) is the integer the layer's quantizer produces.  Without a range: the parameter and its scale.  With
    one: the clamped integers themselves as floats over a unit scale (floor(q / 1) == q exactly, |q| <= 2^24), so that the range
    scan and the packer see no integer outside the range even where floor(P/s) lies outside.  With an element format: the
    elements' encodings, taken the same way over one unit scale."""
    if getattr(nested, "element_format", None) is not None:
        return nested.quantized_integers(param.data, torch.float32), torch.ones(1, dtype=torch.float32, device=param.device)
    if getattr(nested, "q_range", None) is None:
        return param.data, nested.scale.data
    if getattr(nested, "group_size", None) is not None:      # group-wise scales: the clamped integers over ONE unit scale
        return nested.quantized_integers(param.data, torch.float32), torch.ones(1, dtype=torch.float32, device=param.device)
    return nested.quantized_integers(param.data, torch.float32), torch.ones_like(nested.scale.data)


def scale_state(model: torch.nn.Module) -> Dict[str, np.ndarray]:
    out = {}
    for layer in model.modules():
        for attr, tag in (("nested_q_k_layer", "/W_scale"), ("nested_q_w_layer", "/W_scale"), ("nested_q_b_layer", "/b_scale")):
            nested = getattr(layer, attr, None)
            if nested is not None and getattr(nested, "scale", None) is not None and hasattr(layer, "name"):
                out[layer.name + tag] = _host(nested.scale)
                if getattr(nested, "offset", None) is not None:      # asymmetric layers only: other models' files are unchanged
                    out[layer.name + tag.replace("_scale", "_offset")] = _host(nested.offset)
    return out


def save_compress_parameters(model: torch.nn.Module, log_dir: str) -> Dict[str, float]:
    """Writes weights.npy, weights.zip, file_sizes.log (reference format) and scales.npz; returns sizes in MB."""
    os.makedirs(log_dir, exist_ok=True)
    weights_path = os.path.join(log_dir, "weights.npy")
    weights = quantized_state(model)
    for name, layer in model.named_modules():
        if isinstance(layer, (torch.nn.Conv2d, torch.nn.Linear)):            # log_scripts.py:80-82
            weights[name + "/W"] = _host(layer.weight)
            if layer.bias is not None:
                weights[name + "/b"] = _host(layer.bias)
    np.save(weights_path, weights)                                             # pickled dict, like the reference
    zip_file_path = os.path.join(log_dir, "weights.zip")
    with zipfile.ZipFile(zip_file_path, "w", compression=zipfile.ZIP_DEFLATED) as zipf:
        zipf.write(weights_path, arcname="weights.npy")
    np.savez(os.path.join(log_dir, "scales.npz"), **scale_state(model))
    size = os.path.getsize(weights_path) / (1024 * 1024)
    zip_size = os.path.getsize(zip_file_path) / (1024 * 1024)
    with open(os.path.join(log_dir, "file_sizes.log"), "w") as log_file:
        log_file.write(f"Weights size: {size:.4f} MB\n")
        log_file.write(f"Compressed weights size: {zip_size:.4f} MB\n")
    return {"weights_mb": size, "zip_mb": zip_size}


# ------------------------------------------------------------------------------------------------ lossless packed export
# The int8 file above reproduces the reference's artefact and its limits: |q| > 127 wraps, the scales sit in a side file,
# BatchNorm statistics and loss-term buffers are nowhere, and nothing reads it back.  The packed container stores every
# q = floor(P/s) of K1 exactly (bit-packed by lq_q_pack, include/lq_hip.h), the scales, and the rest of the state_dict.
PACKED_FORMAT = "lq-packed"
PACKED_VERSION = 1
PACKED_FILES = ("weights_packed.npz", "weights_packed.zip", "packed_sizes.log")


def _manifest_bytes(manifest: dict) -> np.ndarray:
    return np.frombuffer(json.dumps(manifest).encode("utf-8"), dtype=np.uint8)


def _plain_state_keys(model: torch.nn.Module, tensors) -> List[str]:
    """state_dict keys of everything that is not a quantized parameter or its scale, in state_dict order."""
    skip = {id(p) for _, p, _ in tensors} | {id(nested.scale) for _, _, nested in tensors}
    skip |= {id(nested.offset) for _, _, nested in tensors if getattr(nested, "offset", None) is not None}
    owned = {key for key, p in model.named_parameters() if id(p) in skip}
    return [k for k in model.state_dict().keys() if k not in owned]


def _mx_scales_to_store(tensors) -> Dict[str, np.ndarray]:
    """{name: array} for the tensors with an element format: what the container holds as their scale -- under "e8m0" ONE uint8 per
    group, the exponent of s_eff plus 127 (the E8M0 byte of an MX block); under "fp32" the scale itself.  ValueError naming the
    tensor when a group has no valid scale or an element has no finite value (its code would stand for another value)."""
    out, checks = {}, []
    for name, param, nested in tensors:
        if getattr(nested, "element_format", None) is None:
            continue
        s = _host(nested.scale)
        eff = ops.mx_effective_scale(s, nested.scale_format)
        if not (np.isfinite(eff) & (eff > 0)).all():
            raise ValueError(f"{name}: {int((~(np.isfinite(eff) & (eff > 0))).sum())} groups have no valid {nested.scale_format} scale "
                             "(not positive and finite, subnormal or beyond 2^127): cannot pack it")
        out[name] = (eff.view(np.uint32) >> 23).astype(np.uint8) if nested.scale_format == "e8m0" else s
        fq = ops.fq_forward_mx(param.data, nested.scale.data, nested.element_format, nested.group_size, nested.scale_format)
        checks.append((name, (~torch.isfinite(fq)).sum()))
    if checks:
        for (name, _), n in zip(checks, torch.stack([c for _, c in checks]).tolist()):      # one device->host copy
            if n:
                raise ValueError(f"{name}: {n} elements have no finite value on the element grid (NaN or Inf in the parameter): their "
                                 "NaN code cannot be told from a value's; cannot pack it")
    return out


def _mx_decode(param: torch.Tensor, q: torch.Tensor, s_eff: torch.Tensor, element_format: str, group_size):
    """(P, codes) with the parameter's strides for the stored encodings ``q`` (int32, logical order) of a layer with an element
    format: P = value(code) * s_eff, the value from the format's 2^bits-entry table, s_eff broadcast over its groups in the
    parameter's memory order (a bias: one group)."""
    R, C, axis, gs = init_geometry(tuple(param.shape), param.data.stride(), tuple(s_eff.shape), group_size)
    qs = torch.empty_like(param.data, dtype=torch.int32).copy_(q)
    pr = torch.empty_like(param.data)
    gs = min(gs, R if axis == 0 else C)
    nb = -(-(R if axis == 0 else C) // gs)
    sx = s_eff.reshape((nb, C) if axis == 0 else (R, nb)).repeat_interleave(gs, dim=axis)[:R, :C]
    table = torch.from_numpy(ops.mx_decode_table(element_format)).to(param.device)
    torch.as_strided(pr, (R, C), (C, 1)).copy_(table[torch.as_strided(qs, (R, C), (C, 1)).long()] * sx)
    return pr, qs


def save_packed_parameters(model: torch.nn.Module, log_dir: str) -> Dict[str, float]:
    """Writes weights_packed.npz (manifest, codes, scales, state), weights_packed.zip and packed_sizes.log next to the
    reference export (which it does not touch); returns {"packed_mb", "zip_mb", "bits_per_weight"}.  Raises ValueError naming
    the tensor when an integer cannot be stored exactly (NaN, Inf, |q| beyond int32); then no file is written.
    A tensor with an element format is stored as its encodings, packed at the format's 4 / 6 / 8 bits, with ``element_format``,
    ``scale_format`` and ``group_size`` in its manifest entry and its scales as ``_mx_scales_to_store`` gives them."""
    tensors = quantized_tensors(model)
    if not tensors:
        raise ValueError("the model has no quantized tensor to pack")
    dev = tensors[0][1].device
    mx_scales = _mx_scales_to_store(tensors)
    ranges = torch.empty((len(tensors), 2), dtype=torch.int32, device=dev)
    sources = [_pack_source(param, nested) for _, param, nested in tensors]
    for k, (src, unit) in enumerate(sources):
        ops.q_minmax(src, unit, out=ranges[k])
    lohi = ranges.tolist()                                      # every range in one device->host copy
    entries = []
    for (name, param, nested), (lo, hi) in zip(tensors, lohi):
        if name in mx_scales:      # every code of the format has its place: 0 .. 2^bits - 1
            lo, hi = 0, (1 << ops.check_element_format(nested.element_format).bits) - 1
        if lo > hi:
            raise ValueError(f"{name}: floor(P/s) has no finite integer (NaN/Inf or beyond int32): cannot pack it")
        entries.append({"name": name, "shape": list(param.shape), "scale_shape": list(nested.scale.shape),
                        "orientation": nested.orientation, "qmin": int(lo), "bits": int(hi - lo).bit_length(),
                        "numel": int(param.numel())})
        if getattr(nested, "rounding", "floor") != "floor":      # floor layers get no key: their container is unchanged
            entries[-1]["rounding"] = nested.rounding
        if getattr(nested, "group_size", None) is not None:      # layers without group-wise scales get no key either
            entries[-1]["group_size"] = int(nested.group_size)
        if getattr(nested, "asymmetric", False):                 # nor symmetric layers: the offset array sits behind the scale
            entries[-1]["asymmetric"] = True
        if name in mx_scales:                                    # nor layers without an element format
            entries[-1].update({"element_format": nested.element_format, "scale_format": nested.scale_format})
    bad = torch.zeros(len(tensors), dtype=torch.int64, device=dev)
    words = [ops.q_pack(src, unit, qmin=e["qmin"], bits=e["bits"], bad=bad[k:k + 1])[0]
             for k, ((src, unit), e) in enumerate(zip(sources, entries))]
    for e, nbad in zip(entries, bad.tolist()):
        if nbad:
            raise ValueError(f"{e['name']}: {nbad} elements of floor(P/s) are NaN, Inf or beyond int32: cannot pack it")
    state_keys = _plain_state_keys(model, tensors)
    sd = model.state_dict()
    manifest = {"format": PACKED_FORMAT, "version": PACKED_VERSION, "tensors": entries, "state": state_keys}
    arrays = {"manifest": _manifest_bytes(manifest)}
    for (name, _, nested), e, w in zip(tensors, entries, words):
        arrays[name + ".codes"] = w.cpu().numpy().view(np.uint32)
        arrays[name + ".scale"] = mx_scales[name] if name in mx_scales else _host(nested.scale)
        if e.get("asymmetric"):
            arrays[name + ".offset"] = _host(nested.offset)
    for key in state_keys:
        arrays["state/" + key] = np.array(sd[key].detach().cpu().numpy(), order="C")   # keeps 0-d counters 0-d

    os.makedirs(log_dir, exist_ok=True)
    final = [os.path.join(log_dir, f) for f in PACKED_FILES]
    tmp = [os.path.join(log_dir, "." + f + ".tmp") for f in PACKED_FILES]
    try:
        with open(tmp[0], "wb") as fh:
            np.savez(fh, **arrays)
        with zipfile.ZipFile(tmp[1], "w", compression=zipfile.ZIP_DEFLATED) as zipf:
            zipf.write(tmp[0], arcname=PACKED_FILES[0])
        size = os.path.getsize(tmp[0]) / (1024 * 1024)
        zip_size = os.path.getsize(tmp[1]) / (1024 * 1024)
        n_total = sum(e["numel"] for e in entries)
        bpw = sum(e["numel"] * e["bits"] for e in entries) / n_total
        with open(tmp[2], "w") as log_file:
            log_file.write(f"Packed weights size: {size:.4f} MB\n")
            log_file.write(f"Compressed packed weights size: {zip_size:.4f} MB\n")
            log_file.write(f"Bits per quantised weight: {bpw:.4f}\n")
        for t, f in zip(tmp, final):
            os.replace(t, f)
    finally:
        for t in tmp:
            if os.path.exists(t):
                os.remove(t)
    return {"packed_mb": size, "zip_mb": zip_size, "bits_per_weight": bpw}


def read_packed_manifest(z) -> dict:
    manifest = json.loads(bytes(np.asarray(z["manifest"], dtype=np.uint8)).decode("utf-8"))
    if not isinstance(manifest, dict) or manifest.get("format") != PACKED_FORMAT or manifest.get("version") != PACKED_VERSION:
        raise ValueError(f"not an {PACKED_FORMAT} version {PACKED_VERSION} container: format={manifest.get('format')!r} "
                         f"version={manifest.get('version')!r}" if isinstance(manifest, dict) else "manifest is not an object")
    return manifest


def _check_packed(model: torch.nn.Module, manifest: dict, z, tensors, state_keys) -> None:
    """Every mismatch between the container and the model raises ValueError before anything is changed."""
    entries = manifest.get("tensors", [])
    names = [e.get("name") for e in entries]
    have = [name for name, _, _ in tensors]
    if names != have:
        missing = sorted(set(have) - set(names))
        extra = sorted(set(names) - set(have))
        raise ValueError(f"quantized tensors differ: missing from the container {missing}, not in the model {extra}"
                         + ("" if missing or extra else " (order differs)"))
    for (name, param, nested), e in zip(tensors, entries):
        if list(e.get("shape", [])) != list(param.shape):
            raise ValueError(f"{name}: shape {e.get('shape')} in the container, {list(param.shape)} in the model")
        if e.get("group_size") != getattr(nested, "group_size", None):      # a missing key means no group-wise scales
            raise ValueError(f"{name}: group_size {e.get('group_size')} in the container, {getattr(nested, 'group_size', None)} in "
                             "the model")
        if bool(e.get("asymmetric", False)) != bool(getattr(nested, "asymmetric", False)):      # a missing key means symmetric
            raise ValueError(f"{name}: asymmetric {bool(e.get('asymmetric', False))} in the container, "
                             f"{bool(getattr(nested, 'asymmetric', False))} in the model")
        for key in ("element_format", "scale_format"):      # a missing key means an integer layer
            if e.get(key) != getattr(nested, key, None):
                raise ValueError(f"{name}: {key} {e.get(key)!r} in the container, {getattr(nested, key, None)!r} in the model")
        if list(e.get("scale_shape", [])) != list(nested.scale.shape):
            raise ValueError(f"{name}: scale shape {e.get('scale_shape')} in the container, {list(nested.scale.shape)} in the model")
        if e.get("orientation") != nested.orientation:
            raise ValueError(f"{name}: orientation {e.get('orientation')!r} in the container, {nested.orientation!r} in the model")
        if e.get("rounding", "floor") != getattr(nested, "rounding", "floor"):      # a missing key means floor
            raise ValueError(f"{name}: rounding {e.get('rounding', 'floor')!r} in the container, "
                             f"{getattr(nested, 'rounding', 'floor')!r} in the model")
        bits, numel = e.get("bits"), e.get("numel")
        if not isinstance(bits, int) or not 0 <= bits <= 32 or numel != param.numel():
            raise ValueError(f"{name}: bad bits/numel {bits}/{numel}")
        qmin = e.get("qmin")
        if not isinstance(qmin, int) or qmin < -(2 ** 31) or qmin + (1 << bits) - 1 > 2 ** 31 - 1 and bits < 32:
            raise ValueError(f"{name}: qmin {qmin} with {bits} bits leaves int32")
        codes = z[name + ".codes"] if name + ".codes" in z.files else None
        if codes is None or codes.dtype != np.uint32 or codes.shape != (ops.packed_words(numel, bits),):
            raise ValueError(f"{name}: codes missing or not {ops.packed_words(numel, bits)} uint32 words")
        sc = z[name + ".scale"] if name + ".scale" in z.files else None
        sc_dtype = np.uint8 if e.get("scale_format") == "e8m0" else np.float32
        if sc is None or sc.dtype != sc_dtype or list(sc.shape) != list(nested.scale.shape):
            raise ValueError(f"{name}: scale missing or not {np.dtype(sc_dtype).name} {list(nested.scale.shape)}")
        if e.get("element_format") is not None and (bits != ops.check_element_format(e["element_format"]).bits or qmin != 0):
            raise ValueError(f"{name}: {e['element_format']} codes are stored at {ops.check_element_format(e['element_format']).bits} "
                             f"bits from 0, the container says {bits} bits from {qmin}")
        if e.get("asymmetric"):
            off = z[name + ".offset"] if name + ".offset" in z.files else None
            if off is None or off.dtype != np.float32 or list(off.shape) != list(nested.scale.shape):
                raise ValueError(f"{name}: offset missing or not float32 {list(nested.scale.shape)}")
    if list(manifest.get("state", [])) != state_keys:
        missing = sorted(set(state_keys) - set(manifest.get("state", [])))
        extra = sorted(set(manifest.get("state", [])) - set(state_keys))
        raise ValueError(f"state entries differ: missing from the container {missing}, not in the model {extra}")
    sd = model.state_dict()
    for key in state_keys:
        a = z["state/" + key] if "state/" + key in z.files else None
        if a is None or tuple(a.shape) != tuple(sd[key].shape):
            raise ValueError(f"state entry {key}: missing or shape {None if a is None else a.shape} != {tuple(sd[key].shape)}")


def _restore_groupwise(param: torch.Tensor, q: torch.Tensor, s: torch.Tensor, group_size: int, rounding: str, b=None):
    """(P, q) with the parameter's strides for the stored integers ``q`` (int32, logical order) of a group-wise layer:
    P = (q + 1/2) * s for floor, q * s for nearest, s broadcast by the index rule of include/lq_hip.h (lq_fq_forward_group);
    an asymmetric layer's offset ``b`` is broadcast the same way and added."""
    R, C, axis = group_geometry(tuple(param.shape), param.data.stride(), tuple(s.shape), group_size)
    qs = torch.empty_like(param.data, dtype=torch.int32).copy_(q)
    pr = torch.empty_like(param.data)
    gs = min(int(group_size), R if axis == 0 else C)
    sx = s.repeat_interleave(gs, dim=axis)[:R, :C]
    qm = torch.as_strided(qs, (R, C), (C, 1)).to(torch.float32)      # the memory-order matrix of include/lq_hip.h
    pm = (qm if rounding == "nearest" else qm + 0.5) * sx
    if b is not None:
        pm = pm + b.repeat_interleave(gs, dim=axis)[:R, :C]
    torch.as_strided(pr, (R, C), (C, 1)).copy_(pm)
    return pr, qs


def load_packed_parameters(model: torch.nn.Module, path: str) -> dict:
    """Restores a weights_packed.npz (or the directory holding it) into ``model`` -- built by build_model with the same
    config, either kernel_storage: each quantized P becomes a value whose floor(P/s) is the stored integer, each scale and every
    state entry the stored one, copied into the existing tensors.  A rounding="nearest" layer takes another pre-image: (q + 1/2) * s
    is a tie under rint, so its P becomes q * s, and the layer's own integer view of that P is compared with q on the device.
    A group-wise layer is restored the same way with its scale broadcast over the groups, and always verified through its own view.
    An asymmetric layer takes P = (q + 1/2) * s + b (floor) or q * s + b (nearest) and is verified through the affine forward; a
    container and a model that disagree on ``asymmetric`` raise.
    A layer with an element format takes P = value(code) * s_eff (the value from the format's decode table) and s = s_eff, and its
    own code view of that P is compared with the stored codes on the device; a container and a model that disagree on the element
    format, the scale format or the group size raise.
    Format, version, names, shapes, orientations and roundings are checked first: on a mismatch, or a restored value that does
    not round back, ValueError is raised and the model is left untouched.  Returns the manifest."""
    if os.path.isdir(path):
        path = os.path.join(path, PACKED_FILES[0])
    tensors = quantized_tensors(model)
    with np.load(path, allow_pickle=False) as z:
        manifest = read_packed_manifest(z)
        state_keys = _plain_state_keys(model, tensors)
        _check_packed(model, manifest, z, tensors, state_keys)
        codes = {e["name"]: z[e["name"] + ".codes"] for e in manifest["tensors"]}
        scales = {e["name"]: z[e["name"] + ".scale"] for e in manifest["tensors"]}
        offsets = {e["name"]: z[e["name"] + ".offset"] for e in manifest["tensors"] if e.get("asymmetric")}
        state = {key: z["state/" + key] for key in state_keys}
    if not tensors:
        return manifest
    dev = tensors[0][1].device
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    outside = torch.zeros(1, dtype=torch.int64, device=dev)      # nearest layers: stored integers beyond the model layer's range
    restored = []
    for (name, param, nested), e in zip(tensors, manifest["tensors"]):
        w = torch.from_numpy(codes[name].view(np.int32)).to(dev)
        if e.get("element_format") is not None:
            sc = scales[name]
            s = torch.from_numpy((sc.astype(np.uint32) << 23).view(np.float32) if sc.dtype == np.uint8 else sc).to(dev)
            unit = torch.ones(1, dtype=torch.float32, device=dev)
            _, q, _ = ops.q_unpack(w, 0, e["bits"], unit, param.shape, want_out=False, want_restore=False)
            pr, qs = _mx_decode(param, q, s, e["element_format"], e.get("group_size"))
            view = ops.fq_forward_mx(pr, s, e["element_format"], e.get("group_size"), e["scale_format"], q_dtype=torch.int32)[1]
            bad += (view != qs).sum()
            restored.append((param, nested, s, pr, None))
            continue
        s = torch.from_numpy(scales[name]).to(dev)
        if e.get("group_size") is not None:
            # P = (q + 1/2) * s (floor) or q * s (nearest) with the scale broadcast over its groups in the parameter's memory
            # order; the layer's own group-wise integer view of that P is compared with q on the device
            unit = torch.ones(1, dtype=torch.float32, device=dev)
            _, q, _ = ops.q_unpack(w, e["qmin"], e["bits"], unit, param.shape, want_out=False, want_restore=False)
            b = torch.from_numpy(offsets[name]).to(dev) if e.get("asymmetric") else None
            pr, qs = _restore_groupwise(param, q, s, e["group_size"], e.get("rounding", "floor"), b)
            if b is not None:
                view = ops.fq_forward_group_affine(pr, s, b, *nested.q_range, e["group_size"], q_dtype=torch.int32,
                                                   rounding=nested.rounding)[1]
            else:
                view = ops.fq_forward_group(pr, s, *nested.q_range, e["group_size"], q_dtype=torch.int32, rounding=nested.rounding)[1]
            beyond = (qs < nested.q_range[0]) | (qs > nested.q_range[1])
            outside += beyond.sum()
            bad += ((view != qs) & ~beyond).sum()
        elif e.get("rounding", "floor") == "nearest":
            # rint(fl(fl(q * s) / s)) == q holds for |q| < 2^22 and can miss beyond: counted with the stored scale, like the floor misses
            pr, q, _ = ops.q_unpack(w, e["qmin"], e["bits"], s, param.shape, want_restore=False)
            view = ops.fq_forward_clip(pr, s, *nested.q_range, q_dtype=torch.int32, rounding="nearest")[1]
            beyond = (q < nested.q_range[0]) | (q > nested.q_range[1])      # the layer would clamp these: not a rounding miss
            outside += beyond.sum()
            bad += ((view != q) & ~beyond).sum()
        else:
            _, _, pr = ops.q_unpack(w, e["qmin"], e["bits"], s, param.shape, want_out=False, want_q=False, bad=bad)
        restored.append((param, nested, s, pr, offsets.get(name)))
    nbad, noutside = int(bad.item()), int(outside.item())
    if noutside:
        raise ValueError(f"{noutside} stored integers lie outside the integer range of their layer in the model (the container was "
                         "written by a model with a wider range): model left untouched")
    if nbad:
        raise ValueError(f"{nbad} restored values do not round back to their stored integer (|q| >= 2^22) or code: model left untouched")
    with torch.no_grad():
        for param, nested, s, pr, off in restored:
            param.data.copy_(pr)                               # into the parameter's own storage (HWIO or OIHW order)
            nested.scale.data.copy_(s)
            if off is not None:
                nested.offset.data.copy_(torch.from_numpy(off))
        sd = model.state_dict()
        for key, a in state.items():
            sd[key].copy_(torch.from_numpy(np.array(a, order="C")))
    return manifest
