"""The comparison rule of tests/train_kernel_case.py, proven on the CPU before a GPU sees it.

1. Every case of the GPU table (tests/test_train_kernels_gpu.py) except the 2^20-row one runs with the stand-ins of
   tests/host_emulation.py (fp32 PyTorch rounded to fp16) in the kernel's place: the reference alone stays inside every bound.
2. Deliberate mutants — the mistakes a kernel of this kind can make and a whole-tensor rel-L2 of 4e-3 lets through — are each
   REJECTED by the rule.  The GroupNorm mutants are built into an fp32 restatement of the kernels' own structure (chunk
   partials, per-vector group parameters), which unmutated passes the rule.  A mutant that passes means the rule is too loose.
"""
import pytest
import torch
import torch.nn.functional as F

import host_emulation
import train_kernel_case as tk

CPU = 'cpu'
GN_RUNS = [r for r in tk.gn_runs() if r[:5] != tk.GN_HUGE[:5]]


# ---- 1. the reference alone stays inside every bound ----
@pytest.mark.parametrize('run', GN_RUNS, ids=tk.gn_id)
def test_group_norm_bwd_standin(run):
    tk.run_group_norm_bwd(host_emulation, CPU, run)


@pytest.mark.parametrize('case', tk.LN_CASES, ids=lambda c: f'{c[0]}x{c[1]}-mean{c[2]:g}')
def test_layer_norm_bwd_standin(case):
    tk.run_layer_norm_bwd(host_emulation, CPU, case)


@pytest.mark.parametrize('case', tk.SMB_CASES, ids=lambda c: 'x'.join(str(v) for v in c[:4]) + f'-scale{c[4]:.3f}')
def test_softmax_bwd_standin(case):
    tk.run_softmax_bwd(host_emulation, CPU, case)


@pytest.mark.parametrize('case', tk.GEGLU_CASES, ids=lambda c: f'{c[0]}x{c[1]}')
def test_geglu_standin(case):
    tk.run_geglu(host_emulation, CPU, case)


@pytest.mark.parametrize('n', tk.ACT_SIZES)
def test_activations_standin(n):
    tk.run_activations(host_emulation, CPU, n)


@pytest.mark.parametrize('case', tk.POOL_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_sum_pool_standin(case):
    tk.run_sum_pool(host_emulation, CPU, case)


@pytest.mark.parametrize('C', tk.GATHER_C)
def test_adapter_gather_standin(C):
    tk.run_adapter_gather(host_emulation, CPU, C)


def test_adapter_gather_empty_and_adjoint_standin():
    tk.run_adapter_gather_empty(host_emulation, CPU)
    tk.run_adapter_adjoint(host_emulation, CPU)


@pytest.mark.parametrize('causal', [False, True], ids=['plain', 'causal'])
@pytest.mark.parametrize('ncols', tk.SMR_COLS)
def test_softmax_rows_standin(ncols, causal):
    tk.run_softmax_rows(host_emulation, CPU, ncols, causal)


def test_ulp16():
    v = torch.tensor([0.0, 2.0 ** -24, 2.0 ** -14, 1.0, 1.5, 1.9999, 2.0, 1000.0, 65504.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.5, 32.0], dtype=torch.float64)
    assert torch.equal(tk.ulp16(v), want) and torch.equal(tk.ulp16(-v), want)


# ---- 2. mutants ----
def gnb_chunk_rows(rows, nimg):
    return min(max(rows * nimg // 2048, 8), 512)


def gn_bwd_chunked(dy, x, gamma, beta, groups, eps, nimg, silu=False, x2=None, mutant=None, where=0):
    """vsx_groupnorm_bwd restated in fp32 with the kernels' structure: per-chunk group partials summed in chunk order, group
    parameters looked up per channel of a 16-byte vector, dx = rstd (gz - m1 - xhat m2).  `mutant` breaks one step."""
    xin = (x if x2 is None else torch.cat([x, x2], dim=-1)).float()
    dyf = dy.float().reshape(xin.shape)
    _, rows, C = xin.shape
    cpg = C // groups
    rpc = gnb_chunk_rows(rows, nimg)
    nch = (rows + rpc - 1) // rpc
    ch = torch.arange(C)
    grp = ch // cpg
    lookup = (ch // 8 * 8) // cpg if mutant == 'straddle' else grp      # mutant: the vector's FIRST channel decides the group
    row_in = torch.ones(rows)
    if mutant == 'skip_row':                                           # the last row of chunk `where` never enters a partial
        row_in[min((where + 1) * rpc, rows) - 1] = 0.0

    def group_sums(t):                                                 # [nimg, rows, C] -> [nimg, groups]
        t = F.pad(t * row_in[None, :, None], (0, 0, 0, nch * rpc - rows))
        partial = t.view(nimg, nch, rpc, groups, cpg).sum((2, 4))      # [nimg, nch, groups]
        if mutant == 'drop_chunk':
            partial[:, where] = 0.0
        return partial.sum(1)

    n = float(rows * cpg)
    mean = group_sums(xin) / n
    rstd = ((group_sums(xin * xin) / n - mean * mean).clamp_min(0) + eps).rsqrt()
    xh = (xin - mean[:, None, lookup]) * rstd[:, None, lookup]
    ga, be = gamma.float(), beta.float()
    gz = dyf * ga
    if silu:
        z = xh * ga + be
        sg = torch.sigmoid(z)
        gz = gz * (sg + z * sg * (1.0 - sg))
    m1, m2 = group_sums(gz) / n, group_sums(gz * xh) / n
    core = gz - xh * m2[:, None, lookup] - (0.0 if mutant == 'no_m1' else m1[:, None, lookup])
    dx = rstd[:, None, lookup] * core
    if mutant == 'scale_row':
        dx[nimg - 1, where] *= 1.01
    dx = dx.to(tk.H)
    c1 = x.shape[-1]
    return (dx, None) if x2 is None else (dx[..., :c1].contiguous(), dx[..., c1:].contiguous())


IDLE = (2, 100, 320, 0, 32, 'randn', True)            # cpg = 10, 13 chunks of 8 rows
CONCAT = (2, 77, 640, 320, 32, 'randn', False)        # cpg = 30
CHUNKS = (1, 2100, 32, 0, 8, 'randn', True)           # 263 chunks
GN_MUTANTS = [('skip_row', IDLE, 3), ('skip_row', CHUNKS, 100), ('straddle', IDLE, 0), ('straddle', CONCAT, 0),
              ('drop_chunk', CHUNKS, 259), ('no_m1', IDLE, 0), ('no_m1', CHUNKS, 0), ('scale_row', IDLE, 37),
              ('scale_row', CHUNKS, 2099)]


@pytest.mark.parametrize('run', [IDLE, CONCAT, CHUNKS], ids=tk.gn_id)
def test_chunked_restatement_passes_unmutated(run):
    tk.run_group_norm_bwd(None, CPU, run, fn=gn_bwd_chunked)


def _rejected(what, runner):
    before = len(tk.FIGURES)
    with pytest.raises(AssertionError) as e:
        runner()
    del tk.FIGURES[before:]                                           # a mutant's figures are no parity figures
    name, failed = e.value.args[0][0], e.value.args[0][1]
    assert failed and isinstance(failed, list), e.value                # rejected by the RULE, not by some other assertion
    print(f'mutant {what}: rejected by {failed} ({name})')


@pytest.mark.parametrize('mutant,run,where', GN_MUTANTS, ids=[f'{m}-{tk.gn_id(r)}' for m, r, _ in GN_MUTANTS])
def test_group_norm_bwd_mutant_is_rejected(mutant, run, where):
    def fn(*a, **k):
        return gn_bwd_chunked(*a, mutant=mutant, where=where, **k)
    _rejected(mutant, lambda: tk.run_group_norm_bwd(None, CPU, run, fn=fn))


@pytest.mark.parametrize('case', [(1, 1, 7, 65, 1.0), (2, 8, 9, 77, 40 ** -0.5)], ids=['65', '77'])
def test_softmax_bwd_mutant_is_rejected(case):
    """the row sum misses its last column (column 64: the second trip of the lane loop)"""
    def fn(probs, dprobs, scale):
        p, dp = probs.float(), dprobs.float()
        dprobs.copy_((scale * p * (dp - (dp * p)[..., :-1].sum(-1, keepdim=True))).to(tk.H))
        return dprobs
    _rejected('softmax_bwd row sum without one column', lambda: tk.run_softmax_bwd(None, CPU, case, fn=fn))


def test_layer_norm_bwd_mutant_is_rejected():
    def fn(dy, x, gamma, eps):
        g = host_emulation.layer_norm_bwd(dy, x, gamma, eps).clone()
        g[-1] = (g[-1].float() * 1.01).to(tk.H)                        # the last row (a workgroup's tail) off by 1 %
        return g
    _rejected('layer_norm_bwd last row x 1.01', lambda: tk.run_layer_norm_bwd(None, CPU, (1001, 320, 0.5), fn=fn))
