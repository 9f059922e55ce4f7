"""Test helper: the MLP kernels' network outputs against a float64 evaluation of the same module.

Reference: a deep copy of the module cast to float64 on the CPU, evaluated on the kernel's own inputs. Every
element's error is measured against its own scale

    A = the same network in float64 with every weight, bias and input replaced by its absolute value and
        every activation by the identity (BatchNorm folded into the Linear in front of it, as the kernels hold it),

the quantity an f32 evaluation's rounding error is proportional to (tests/test_gpu_split_range.py's form). Bound:
max |err| / A of the kernel at most 4 x that of torch's own f32 CPU evaluation of the module on the same inputs
(both are f32 and differ in summation order only) and never above 2^-16, the project's bound for the less precise
split-fp16 paths. Decoded rewards and values: rtol 1e-4, atol 1e-5 x support scale against the float64 decode.
Both ratios are printed per shape and, where LZM_REPORT_DIR is set, collected in mlp_shapes_error.json.
"""
import copy
import json
import os

import torch
import torch.nn.functional as F

TOL = 2.0 ** -16
MARGIN = 4.0


def inverse_scalar_transform64(logits, scale, eps=0.001):
    """float64 restatement of InverseScalarTransform (scaling_transform.py:118-128) on Linear logits"""
    p = torch.softmax(logits.double(), dim=1)
    support = torch.arange(-scale, scale + 1, dtype=torch.float64)
    v = (p * support).sum(1)
    tmp = (torch.sqrt(1 + 4 * eps * (v.abs() + 1 + eps)) - 1) / (2 * eps)
    return torch.sign(v) * (tmp * tmp - 1)


def _ratio(x, ref, A):
    return float(((x.double() - ref).abs() / A.clamp_min(1e-300)).max())


def report(name, entries):
    """entries: {tensor name: (kernel ratio, torch f32 ratio)}"""
    print(f"{name}: max |err| / A, kernel vs torch f32: " +
          "; ".join(f"{k} {a:.2e} vs {b:.2e}" for k, (a, b) in entries.items()))
    out = os.environ.get("LZM_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "mlp_shapes_error.json")
        rep = json.load(open(path)) if os.path.exists(path) else {}
        rep[name] = {k: dict(kernel=a, torch_f32=b) for k, (a, b) in entries.items()}
        with open(path, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)


def check_scaled(name, tensors):
    """tensors: {tensor name: (kernel output, float64 reference, scale A, torch f32 output)}"""
    entries = {}
    for k, (got, ref, A, f32) in tensors.items():
        got, ref, A, f32 = got.detach().cpu(), ref.detach().cpu().double(), A.detach().cpu().double(), f32.detach().cpu()
        assert torch.isfinite(got).all(), (name, k)
        entries[k] = (_ratio(got, ref, A), _ratio(f32, ref, A))
    report(name, entries)
    for k, (a, b) in entries.items():
        assert a <= MARGIN * b, f"{name} {k}: kernel {a:.3e} > {MARGIN} x torch f32 {b:.3e}"
        assert a <= TOL, f"{name} {k}: kernel {a:.3e} > 2^-16"
    return entries


def recurrent_scale(model, lat, act):
    """A of (next latent, policy logits) for recurrent_inference(lat, act): lat float64 [n, H], act int64 [n]"""
    from lightzero_amd.fused import describe
    layers, dims = describe(model)
    W = [(w.detach().cpu().double().abs(), b.detach().cpu().double().abs()) for (w, b), _ in layers]
    lin = lambda x, l: F.linear(x, W[l][0], W[l][1])
    x = torch.cat((lat.abs(), F.one_hot(act, dims["actions"]).double()), dim=1)
    nxt = lin(lin(x, 0), 1)
    off = 2
    if dims["res"]:
        nxt = nxt + lat.abs()
        off = 4
    p = lin(lin(nxt, off + 2), off + 3)
    return nxt, lin(lin(p, off + 6), off + 7)


def check_search_network(name, r, S, B, scale):
    """the fused search r's filed latents, recorded policy logits and decoded scalars (tests/test_gpu_fused.py's
    fused_search) against float64 on the latents it gathered and the actions it recorded"""
    model, rec = r["model"], r["rec"]
    pool = r["pool"].cpu()
    A = rec["policy_logits"].shape[-1]
    x = torch.from_numpy(rec["x"]).long()
    idx = torch.arange(B)
    lat = torch.stack([pool[x[k], idx] for k in range(S)]).reshape(S * B, -1)
    act = torch.from_numpy(rec["action"]).long().reshape(S * B)
    with torch.no_grad():
        ref = copy.deepcopy(model).cpu().double().eval().recurrent_inference(lat.double(), act)
        f32 = copy.deepcopy(model).cpu().float().eval().recurrent_inference(lat, act)
        a_lat, a_pol = recurrent_scale(model, lat.double(), act)
    out = check_scaled(name, dict(
        latent=(pool[1:S + 1].reshape(S * B, -1), ref.latent_state, a_lat, f32.latent_state),
        policy=(torch.from_numpy(rec["policy_logits"]).reshape(S * B, A), ref.policy_logits, a_pol, f32.policy_logits)))
    dec = torch.from_numpy(rec["decoded"]).reshape(S * B, 2)
    torch.testing.assert_close(dec[:, 0], inverse_scalar_transform64(ref.reward, scale).float(), rtol=1e-4,
                               atol=1e-5 * scale)
    torch.testing.assert_close(dec[:, 1], inverse_scalar_transform64(ref.value, scale).float(), rtol=1e-4,
                               atol=1e-5 * scale)
    return out


def check_initial_network(name, model, obs, got):
    """initial_inference outputs `got` of a kernel on `obs` against float64. The scaled form runs up to the
    pre-SimNorm activations (GELU as the identity); the latent after SimNorm is compared directly, each element
    against the largest pre-SimNorm scale of its group (a softmax moves by at most half its inputs' largest
    change) plus 2^-4 for the few-ulp rounding of the exponentials and the division of values <= 1. The
    prediction network is one more kernel stage: its reference and scale take the kernel's own latent as input."""
    from lightzero_amd.initial import describe_initial
    layers, dims = describe_initial(model)
    W = [(w.detach().cpu().double().abs(), b.detach().cpu().double().abs()) for w, b in layers]
    lin = lambda x, l: F.linear(x, W[l][0], W[l][1])
    obs = obs.detach().cpu().float()
    n, G = obs.shape[0], dims["group"]
    lat = got.latent_state.detach().cpu().float()
    with torch.no_grad():
        m64 = copy.deepcopy(model).cpu().double().eval()
        m32 = copy.deepcopy(model).cpu().float().eval()
        m64.representation_network.sim_norm.dim = m32.representation_network.sim_norm.dim = G
        ref_lat, f32_lat = m64.representation_network(obs.double()), m32.representation_network(obs)
        ref_pol, ref_val = m64.prediction_network(lat.double())
        f32_pol, f32_val = m32.prediction_network(lat)
    pre = lin(lin(obs.double().abs(), 0), 1)
    a_lat = pre.view(n, -1, G).max(dim=-1, keepdim=True).values.expand(n, pre.shape[1] // G, G).reshape(n, -1) + 2.0 ** -4
    p = lin(lin(lat.double().abs(), 2), 3)
    return check_scaled(name, dict(latent=(lat, ref_lat, a_lat, f32_lat),
                                   value=(got.value, ref_val, lin(lin(p, 4), 5), f32_val),
                                   policy=(got.policy_logits, ref_pol, lin(lin(p, 6), 7), f32_pol)))
