"""CPU tests of what the HMM entry points refuse on the host, before any HIP call:
  * the return codes of svae_hmm_estep_f64 (include/svae_hip.h), the one public HMM entry whose numbering is older than
    the shared prefix of csrc/hmm_units.hpp: no -4, B == 0 answered only after the pointers, one code for a NULL or a short
    workspace;
  * the shape refusals of hmm_estep, hmm_viterbi, hmm_sample and hmm_estep_vjp (svae_amd/hmm/hmm_inference.py), which are
    judged from shapes alone: no library is loaded and no device is asked for."""
import ctypes

import numpy as np
import pytest


def test_estep_rejects_bad_arguments_on_the_host_with_its_own_codes():
    """every argument error comes back before any HIP call (safe without a GPU)"""
    from svae_amd import _lib as L
    lib = L.load()
    raw = (ctypes.c_double * 1024)()
    p = ctypes.c_void_p(ctypes.addressof(raw))        # a host address: must never be dereferenced
    need = lib.svae_hmm_workspace_bytes(2, 3, 5)
    assert need > 0

    def call(B=2, T=3, K=5, pb=0, init=p, pair=p, node=p, logZ=p, E_init=p, E_trans=p, E_states=p, ws=p, ws_bytes=need):
        return lib.svae_hmm_estep_f64(B, T, K, pb, init, pair, node, logZ, E_init, E_trans, E_states, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(node=None) == -7
    assert call(logZ=None) == -8
    assert call(E_init=None) == -9
    assert call(E_trans=None) == -10
    assert call(E_states=None) == -11
    assert call(ws=None) == -12
    assert call(ws_bytes=need - 1) == -12 and call(ws_bytes=0) == -12       # one code: NULL or too small
    # there is no -4: pair_batched is a truth value here (not 0 = per-sequence), whatever the bad argument behind it
    assert call(pb=2, init=None) == -5 and call(pb=-1, ws=None) == -12
    # the first failing check decides
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=65, init=None) == -3
    assert call(init=None, pair=None, node=None) == -5 and call(node=None, logZ=None, ws=None) == -7
    assert call(E_init=None, E_trans=None, E_states=None) == -9 and call(E_states=None, ws=None) == -11
    codes = {call(B=-1), call(T=0), call(K=0), call(init=None), call(pair=None), call(node=None), call(logZ=None),
             call(E_init=None), call(E_trans=None), call(E_states=None), call(ws=None)}
    assert codes == {-1, -2, -3, -5, -6, -7, -8, -9, -10, -11, -12}
    # B == 0 returns 0 only after every pointer, the workspace's included (an empty batch needs no bytes)
    assert call(B=0, ws_bytes=0) == 0 and call(B=0, pb=1, ws_bytes=0) == 0
    assert call(B=0, T=0) == -2 and call(B=0, K=65) == -3
    for i, name in enumerate(("init", "pair", "node", "logZ", "E_init", "E_trans", "E_states")):
        assert call(B=0, **{name: None}) == -5 - i, name
    assert call(B=0, ws=None, ws_bytes=0) == -12


def _estep(nat):
    from svae_amd.hmm.hmm_inference import hmm_estep
    return hmm_estep(nat)


def _viterbi(nat):
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    return hmm_viterbi(nat)


def _sample(nat):
    from svae_amd.hmm.hmm_inference import hmm_sample
    return hmm_sample(nat, num_samples=2)


def _vjp(nat):
    from svae_amd.hmm.hmm_inference import hmm_estep_vjp
    return hmm_estep_vjp(nat, (None, (None, None, None)))


def _z(*shape):
    return np.zeros(shape)


NODE_RANK = "node_params must be"
K_RANGE = "number of states K="
NO_STEPS = "node_params has no steps"
MISMATCH = "init/pair parameter shapes do not match the node potentials"
# B = 2, T = 4, K = 3 wherever the case does not say otherwise
REFUSALS = [
    ("node_rank_1", (_z(3), _z(3, 3), _z(3)), NODE_RANK),
    ("node_rank_4", (_z(3), _z(3, 3), _z(2, 2, 4, 3)), NODE_RANK),
    ("K_0", (_z(0), _z(0, 0), _z(2, 4, 0)), K_RANGE),
    ("K_65", (_z(65), _z(65, 65), _z(2, 4, 65)), K_RANGE),
    ("T_0", (_z(3), _z(3, 3), _z(2, 0, 3)), NO_STEPS),
    ("T_0_unbatched", (_z(3), _z(3, 3), _z(0, 3)), NO_STEPS),
    ("init_shape", (_z(4), _z(3, 3), _z(2, 4, 3)), MISMATCH),
    ("init_rank", (_z(1, 3), _z(3, 3), _z(2, 4, 3)), MISMATCH),
    ("pair_shape", (_z(3), _z(3, 4), _z(2, 4, 3)), MISMATCH),
    ("pair_rank_1", (_z(3), _z(3), _z(2, 4, 3)), MISMATCH),
    ("pair_rank_4", (_z(3), _z(2, 1, 3, 3), _z(2, 4, 3)), MISMATCH),
    ("pair_batch", (_z(3), _z(5, 3, 3), _z(2, 4, 3)), MISMATCH),
    ("pair_batch_unbatched_node", (_z(3), _z(2, 3, 3), _z(4, 3)), MISMATCH),
]


@pytest.mark.parametrize("fn", [_estep, _viterbi, _sample, _vjp], ids=["estep", "viterbi", "sample", "estep_vjp"])
@pytest.mark.parametrize("nat,message", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_shape_refusals_come_before_the_library_and_the_device(fn, nat, message, monkeypatch):
    import torch
    from svae_amd import _lib as L

    def touched(*a, **k):
        raise AssertionError("a shape refusal must not load the library or ask for a device")

    monkeypatch.setattr(L, "load", touched)
    monkeypatch.setattr(torch.cuda, "current_device", touched)
    for as_tensor in (False, True):
        args = tuple(torch.as_tensor(x) for x in nat) if as_tensor else nat
        with pytest.raises(ValueError, match=message):
            fn(args)
