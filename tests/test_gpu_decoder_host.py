"""GPU: the host side of the decoder handle (decoder.hip below ``validate``), through the raw binding.

Two models: the 16-channel any-shape one (``CFG1``: ``k_decode`` / ``k_decode_batch``) and a 32/256-channel model of 2 x 5
layers without biases, the shape of the specialised kernels (one workgroup for a single step, nine for a run or a batch).
Every handle of a model is loaded from one prefill over one random prompt, so two handles of a model start from the same
state and equality is bit for bit.

On the parent of the commit that added this file, every test here passes unmodified except the two cases of
``test_a_refused_update_changes_nothing``: there a refused update had already overwritten the layers before the NULL one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from wavenet_amd import FasterWaveNet, _lib
from wavenet_amd._lib import check, ptr, ptr_array

from gpu_util import CFG1, CFG2, build, dev

pytestmark = pytest.mark.gpu

NINE = dict(CFG2, residual_conv_channels=[32] * 5, residual_num_blocks=2)
CFGS = {"any-shape": CFG1, "nine-workgroup": NINE}
Q, FIRST, HOP, PHASE = 256, 7, 4, 1
_MODELS = {}


class _Model(object):
    """A model, a second one of the same shape with other weights, one prompt, the prefill over it, 16 uniforms."""

    def __init__(self, name):
        self.net = build(CFGS[name], cls=FasterWaveNet)[2]
        self.other = build(CFGS[name], seed=4321, cls=FasterWaveNet)[2]
        assert self.net._nine_workgroup_shape(_lib.default_exec_flags()) == (name == "nine-workgroup")
        rs = np.random.RandomState(len(name))
        self.tok = dev(rs.randint(0, Q, (1, self.net.input_width)).astype(np.int32))
        self.net.keep_window = False
        with torch.no_grad():
            self.net.forward_one_step(self.tok)
        self.causal_outs = [t.contiguous() for t in self.net._last_causal_outputs]
        self.layer_ins = list(self.net._last_layer_inputs)
        self.u = dev(rs.random_sample(16))
        self.n_layers = len(self.net._flat_layers)
        self.row = sum(2 * lay.cd for lay in self.net._flat_layers)
        self.table = dev((rs.standard_normal((8, self.row + 4)) * 0.5).astype(np.float32))     # rows 4 floats of padding apart


def model(name):
    if name not in _MODELS:
        _MODELS[name] = _Model(name)
    return _MODELS[name]


class handles(object):
    """``with handles(M) as new:`` -- ``new(...)`` creates a handle of M's model and loads the prompt's state; every handle
    is destroyed on the way out."""

    def __init__(self, M):
        self.M, self.made = M, []

    def __enter__(self):
        return self.new

    def new(self, step_limit=0, rows=0, interp=0):
        M = self.M
        d, keep = M.net._desc(None, (M.table[:rows], HOP, PHASE) if rows else None, step_limit)
        d.frame_interp = interp
        h = C.c_void_p()
        check(_lib.lib().wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
        self.made.append(h)
        load(M, h)
        return h

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        for h in self.made:
            _lib.lib().wn_decoder_destroy(h)


def load(M, h):
    check(_lib.lib().wn_decoder_load_state(h, ptr(M.tok), int(M.tok.shape[1]), ptr_array(M.causal_outs), ptr_array(M.layer_ins), None),
          "wn_decoder_load_state")


def run(h, n, u, first=FIRST):
    """wn_decoder_run -> (rc, message, tokens, probability trace)."""
    lib = _lib.lib()
    out = torch.full((n,), -1, device="cuda", dtype=torch.int32)
    probs = torch.zeros((n, Q), device="cuda")
    rc = lib.wn_decoder_run(h, first, ptr(u), n, ptr(out), ptr(probs), None)
    msg = lib.wn_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, out, probs


def step(h, token=FIRST):
    lib = _lib.lib()
    row = torch.zeros((Q,), device="cuda")
    rc = lib.wn_decoder_step(h, token, ptr(row), 1, None)
    msg = lib.wn_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, row


def run_batch(hs, n, u, firsts):
    lib = _lib.lib()
    N = len(hs)
    toks = [torch.full((n,), -1, device="cuda", dtype=torch.int32) for _ in range(N)]
    probs = [torch.zeros((n, Q), device="cuda") for _ in range(N)]
    rc = lib.wn_decoder_run_batch((C.c_void_p * N)(*[h.value for h in hs]), N, (C.c_int32 * N)(*firsts), ptr_array([u] * N), n,
                                  ptr_array(toks), ptr_array(probs), 0, None)
    msg = lib.wn_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, toks, probs


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", list(CFGS))
def test_a_refused_update_changes_nothing(name):
    """wn_decoder_update_weights with the other model's pointers and a NULL ``Wf`` of the last layer is refused before any
    device work: the handle then decodes the 16 steps of its own model, tokens and trace bit for bit.  (The same update with
    the pointer in place is taken, and shows: the other model's 16 steps differ.)"""
    M = model(name)
    lib = _lib.lib()
    with handles(M) as new:
        rc, msg, t_want, p_want = run(new(), 16, M.u)
        assert rc == 0, msg
        h = new()
        last = M.n_layers - 1
        d, keep = M.other._desc()
        keep["Wf"][last] = None
        rc = lib.wn_decoder_update_weights(h, C.byref(d), None)
        assert rc == _lib.WN_EARG and lib.wn_last_error().decode() == "decoder: layer %d has a NULL weight" % last
        rc, msg, t, p = run(h, 16, M.u)
        assert rc == 0, msg
        assert torch.equal(t, t_want) and same_bits(p, p_want)
        assert lib.wn_decoder_status(h, None) == _lib.WN_OK
        d, keep = M.other._desc()
        check(lib.wn_decoder_update_weights(h, C.byref(d), None), "wn_decoder_update_weights")
        load(M, h)
        rc, msg, t, p = run(h, 16, M.u)
        assert rc == 0 and not same_bits(p, p_want)


def _every_path_once(M, h, partner, nxt):
    """wn_decoder_step, wn_decoder_run of 3 steps, wn_decoder_run_batch of 2 with ``partner``: 6 steps on ``h``.  The run is fed
    ``nxt`` (the step draws nothing), the batched run the run's last token.  -> the 6 probability rows, the tokens of steps
    1 .. 5."""
    rc, msg, row = step(h)
    assert rc == 0, msg
    rc, msg, t, p = run(h, 3, M.u[1:], first=nxt)
    assert rc == 0, msg
    rc, msg, ts, ps = run_batch([h, partner], 2, M.u[4:], [int(t[2]), FIRST])
    assert rc == 0, msg
    assert _lib.lib().wn_decoder_status(h, None) == _lib.WN_OK
    return torch.cat([row[None], p, ps[0]]), t.tolist() + ts[0].tolist()


@pytest.mark.parametrize("name", list(CFGS))
def test_every_path_advances_the_one_counter(name):
    """A handle with ``step_limit = 7`` after one step, a run of 3 and a batched run of 2: a run of 2 more is refused with
    "6 steps run", a run of 1 is taken, and the next batched run finds all 7 steps run.  On the any-shape model, where every
    entry point runs the one step loop, the 7 steps made this way are also the 7 steps of one run on an unlimited handle, bit
    for bit (the ring position counts with them); on the other model a single step runs on one workgroup and a run on nine,
    whose sums are ordered differently, so only the counts are held there."""
    M = model(name)
    with handles(M) as new:
        rc, msg, t_ref, p_ref = run(new(), 7, M.u)
        assert rc == 0, msg
        h, partner = new(step_limit=7), new()
        rows, toks = _every_path_once(M, h, partner, int(t_ref[0]))
        rc, msg, t, p = run(h, 2, M.u[6:], first=toks[-1])
        assert rc == _lib.WN_EARG and msg == ("wn_decoder_run: n = 2 more steps would pass step_limit = 7 (6 steps run since it was "
                                               "set)"), msg
        assert int(t.max()) == -1 and float(p.abs().max()) == 0.0                    # nothing ran
        rc, msg, t, p = run(h, 1, M.u[6:], first=toks[-1])
        assert rc == 0, msg
        rc, msg, ts, ps = run_batch([h, partner], 2, M.u[7:], [int(t[0]), FIRST])
        assert rc == _lib.WN_EARG and "utterance 0 has run all 7 steps of its step_limit" in msg, msg
        assert int(ts[1].max()) == -1
        if name == "any-shape":
            assert toks + t.tolist() == t_ref[1:].tolist() and same_bits(torch.cat([rows, p]), p_ref)


def test_every_path_advances_the_frame_tables_counter():
    """The same calls on an any-shape handle that holds a frame table of hop 4, phase 1 and the 2 rows that 7 steps read
    (positions 1 .. 7): the overrun text of every entry point names the row it would read and the steps run, and the 7 steps
    are those of one run on a handle with a longer table."""
    M = model("any-shape")
    text = "%s: %d more steps would read row 2 of a frame table of 2 rows (hop 4, phase 1, %d steps run on it)"
    with handles(M) as new:
        rc, msg, t_ref, p_ref = run(new(rows=8), 7, M.u)
        assert rc == 0, msg
        h, partner = new(rows=2), new(rows=8)
        rows, toks = _every_path_once(M, h, partner, int(t_ref[0]))
        rc, msg, t, p = run(h, 2, M.u[6:], first=toks[-1])
        assert rc == _lib.WN_EARG and msg == text % ("wn_decoder_run", 2, 6), msg
        assert int(t.max()) == -1 and float(p.abs().max()) == 0.0
        rc, msg, t, p = run(h, 1, M.u[6:], first=toks[-1])
        assert rc == 0, msg
        rc, msg, ts, ps = run_batch([h, partner], 2, M.u[7:], [int(t[0]), FIRST])
        assert rc == _lib.WN_EARG and msg == text % ("wn_decoder_run_batch", 2, 7), msg
        rc, msg, row = step(h)
        assert rc == _lib.WN_EARG and msg == text % ("wn_decoder_step", 1, 7), msg
        assert toks + t.tolist() == t_ref[1:].tolist() and same_bits(torch.cat([rows, p]), p_ref)
        assert not same_bits(p_ref, run(new(), 7, M.u)[3])                          # the table reaches the rows


# the nine-workgroup model: a run of one step is the one-workgroup kernel, wn_decoder_step's; a longer run is on nine
# workgroups, whose sums are ordered differently (WN_DECODER_ONE_WORKGROUP in the header: ~1e-7), so n = 1 only
@pytest.mark.parametrize("name,n,rows,interp", [("any-shape", 1, 0, 0), ("any-shape", 4, 0, 0), ("nine-workgroup", 1, 0, 0),
                                                ("any-shape", 4, 3, 0), ("any-shape", 4, 3, 1)])
def test_wn_decoder_step_is_wn_decoder_runs_first_step(name, n, rows, interp):
    """From one loaded state, the probability row of wn_decoder_step(apply_softmax = 1) is row 0 of wn_decoder_run's trace,
    bit for bit; with a frame table (hop 4, phase 1: step 0 interpolates with alpha = 1/4) in both interpolation modes."""
    M = model(name)
    with handles(M) as new:
        rc, msg, row = step(new(rows=rows, interp=interp))
        assert rc == 0, msg
        rc, msg, t, p = run(new(rows=rows, interp=interp), n, M.u)
        assert rc == 0, msg
        assert same_bits(row, p[0]) and abs(float(row.sum()) - 1.0) < 1e-5
        if rows:                                                                     # the table, and its mode, reach the row
            assert not same_bits(row, step(new())[2])
            assert not same_bits(row, step(new(rows=rows, interp=1 - interp))[2])
