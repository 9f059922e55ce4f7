"""CPU: what conv_infer.StochasticConvNet hands to lzm_smz_conv_net_prepare (fold_stochastic_conv: the BN-folded
convolutions, the option plane's edge maps, the folded FC1) evaluated with plain torch in float64, against the
conv StochasticMuZeroModel's own float64 recurrent_inference through both kinds."""
import copy

import pytest
import torch
import torch.nn.functional as F


def make_model(nres, A, C, V=21, seed=0, **kw):
    from lightzero_amd.model_conv import StochasticMuZeroModel
    torch.manual_seed(seed)
    m = StochasticMuZeroModel((16, 4, 4), A, C, num_res_blocks=nres, reward_support_size=V, value_support_size=V,
                              last_linear_layer_init_zero=False, **kw)
    with torch.no_grad():  # non-trivial BatchNorm statistics so the folding is exercised
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                mod.running_mean.uniform_(-0.2, 0.2), mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5), mod.bias.uniform_(-0.1, 0.1)
    return m.eval()


def boards(n, seed=1):
    """random one-hot 2048 boards [n, 16, 4, 4]"""
    g = torch.Generator().manual_seed(seed)
    return F.one_hot(torch.randint(0, 16, (n, 4, 4), generator=g), 16).permute(0, 3, 1, 2).float()


def eval_set(s, state, option):
    """one kind's half from its folded tensors: (next latent, {head: logits})"""
    head = lambda x, h: F.linear(F.relu(F.linear(F.relu(F.conv2d(x, h[0].reshape(16, 64, 1, 1), h[1])).flatten(1),
                                                 h[2], h[3])), h[4], h[5])
    conv = lambda x, wb: F.conv2d(x, wb[0], wb[1], padding=1)
    plane = (option.float() / s["space"]).to(state.dtype).reshape(-1, 1, 1, 1)
    x = F.relu(conv(state, s["convs"][0]) + plane * s["edge"].t().reshape(1, 64, 4, 4) + state)
    out, blocks = {}, s["convs"][1:]
    for j in range(0, len(blocks), 2):
        if j == len(blocks) // 2:
            nxt = x
        x = F.relu(conv(F.relu(conv(x, blocks[j])), blocks[j + 1]) + x)
    if "reward" in s["heads"]:
        out["reward"] = head(nxt, s["heads"]["reward"])
    out["value"], out["policy"] = head(x, s["heads"]["value"]), head(x, s["heads"]["policy"])
    return nxt, out


@pytest.mark.parametrize("A,C", [(4, 32), (3, 5)])
@pytest.mark.parametrize("nres", [1, 2])
def test_folded_tensors_reproduce_the_module(nres, A, C):
    from lightzero_amd.conv_infer import fold_stochastic_conv
    m = copy.deepcopy(make_model(nres, A, C)).double()
    sets, dims = fold_stochastic_conv(m)
    assert dims == dict(nres=nres, A=A, C=C, V=21)
    with torch.no_grad():
        state = m.representation_network(boards(6).double())
        for afterstate in (False, True):
            opt = torch.arange(6) % (C if afterstate else A)
            want = m.recurrent_inference(state, opt, afterstate=afterstate)
            nxt, got = eval_set(sets[0 if afterstate else 1], state, opt)
            pairs = [(nxt, want.latent_state), (got["value"], want.value), (got["policy"], want.policy_logits)]
            if afterstate:
                pairs.append((got["reward"], want.reward))
            for g, w in pairs:
                assert g.shape == w.shape and float((g - w).abs().max()) <= 1e-12 * float(w.abs().max())


@pytest.mark.parametrize("kw", [dict(observation_shape=(16, 6, 6)), dict(categorical_distribution=False)])
def test_refused_model_raises_not_packable(kw):
    from lightzero_amd.conv_infer import fold_stochastic_conv
    from lightzero_amd.fused import NotPackable
    from lightzero_amd.model_conv import StochasticMuZeroModel
    with pytest.raises(NotPackable):
        fold_stochastic_conv(StochasticMuZeroModel(**kw).eval())
