"""``RnnAgent`` (exp2's o='mlp', c=None arm) against tests/golden/agent_rnn.npz, recorded from the reference's own RnnAgent
(algos/madrqn/agents/rnn_agents.py) by tests/golden/make_golden_exp2.py: state_dict names, shapes and parameters() order on the CPU;
forward and backward on the GPU.  And ``MultiAgentQLearner._build_agent``'s choice of arm (learner.py:64-67)."""
import ast
import math
import os
import types

import numpy as np
import pytest
import torch as th

from oracle.closed_form import closed_form_tensor
from tests.util import assert_close, grad_close

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agent_rnn.npz")
CONFIGS = [(1, False), (2, False), (1, True), (2, True)]
H, F, A = 32, 31, 5


def _args(n_layers, dueling, **kw):
    return types.SimpleNamespace(n_layers=n_layers, hidden_size=H, dueling=dueling, **kw)


def _fixture(n_layers, dueling):
    z = np.load(GOLDEN)
    key = f"L{n_layers}_d{int(dueling)}/"
    return {k[len(key):]: z[k] for k in z.files if k.startswith(key)}


def _closed_form_params(fx):
    params = {}
    for i, (n, s) in enumerate(zip(fx["param_names"], fx["param_shapes"])):
        shape = ast.literal_eval(str(s))
        params[str(n)] = closed_form_tensor(shape, 1.0 + i * math.pi / 7, 0.1 if len(shape) == 1 else 0.25, th.float64)
    return params


@pytest.mark.parametrize("n_layers,dueling", CONFIGS)
def test_state_dict_layout_matches_the_reference(n_layers, dueling):
    from uav_bs_ctrl_amd import REGISTRY, RnnAgent
    assert REGISTRY["rnn"] is RnnAgent
    fx = _fixture(n_layers, dueling)
    net = RnnAgent(F, A, _args(n_layers, dueling))
    assert [n for n, _ in net.named_parameters()] == [str(s) for s in fx["param_names"]]
    assert [str(tuple(p.shape)) for p in net.parameters()] == [str(s) for s in fx["param_shapes"]]
    assert list(net.state_dict().keys()) == [str(s) for s in fx["state_dict_names"]]
    net.load_state_dict({k: v.float() for k, v in _closed_form_params(fx).items()})     # a reference checkpoint loads
    assert net.init_hidden().shape == (1, H) and not net.init_hidden().is_cuda


class _Self:
    def __init__(self, **kw):
        self.obs_shape, self.n_actions = 31, A
        self.args = types.SimpleNamespace(n_layers=1, hidden_size=H, dueling=False, n_heads=4, msg_size=8, key_size=8, n_rounds=1, **kw)


@pytest.mark.parametrize("o,c,want", [("mlp", None, "rnn"), ("mlp", "tarmac", "gnn"), ("mlp", "disc", "gnn"), (None, None, "gnn"),
                                      ("gnn", None, "gnn"), ("absent", None, "gnn")])
def test_build_agent_picks_the_rnn_arm_only_for_mlp_without_comm(o, c, want):
    from uav_bs_ctrl_amd.agents import GnnAgent, RnnAgent
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    s = _Self(c=c) if o == "absent" else _Self(c=c, o=o)
    if want == "gnn" and o in (None, "absent", "gnn"):
        s.obs_shape = dict(agent=2, ubs=2, gt=4)
    net = MultiAgentQLearner._build_agent(s)
    assert type(net) is (RnnAgent if want == "rnn" else GnnAgent)


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers,dueling", CONFIGS)
def test_gpu_forward_and_backward_match_the_reference(n_layers, dueling):
    from uav_bs_ctrl_amd import RnnAgent
    fx = _fixture(n_layers, dueling)
    net = RnnAgent(F, A, _args(n_layers, dueling))
    net.load_state_dict({k: v.float() for k, v in _closed_form_params(fx).items()})
    net = net.cuda()
    f = lambda k: th.as_tensor(fx[k], dtype=th.float32, device="cuda")  # noqa: E731
    h = f("h").requires_grad_(True)
    q, h2 = net(f("x"), h)
    ((q * f("wq")).sum() + (h2 * f("wh")).sum()).backward()
    assert_close(q, th.as_tensor(fx["q"]), 1e-5, "rnn q")
    assert_close(h2, th.as_tensor(fx["h2"]), 1e-5, "rnn h'")
    grad_close(h.grad, th.as_tensor(fx["grad:h"]), "rnn grad h")
    for name, p in net.named_parameters():
        grad_close(p.grad, th.as_tensor(fx["grad:" + name]), f"rnn grad {name}")
