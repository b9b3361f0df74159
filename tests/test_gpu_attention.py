"""``attention_mfma_kernel`` / ``attention_row_kernel`` alone, through
``tvr_attention``, against the fp64 reference of tests/attention_cases.py.

The primitive calls ``launch_attention`` as a block does, so the kernel form is
the engine's choice: key tiles in registers from the launch's longest T (NKT 1 /
2 / 4 / 8, or the chunked online softmax beyond 128), ``TVR_ATT_STAGE`` 0 / 1 / 2
at NKT 1, ``TVR_ATT_VSTAGE`` 0 / 1 at NKT 2 (STAGE 3), and the single-query
kernel for the sequences from ``row_from`` on (``TVR_ROW_ATTN``; refused for 6
and 3 heads, where they stay on the tile kernel).  One small model per
(d_head, n_heads) of attention_cases.MODELS; its weights are never used.  The
rotary tables are passed in (TL's fp32 tables) and go into the reference too.

Every launch (``launch``) checks what must NOT be written, bit for bit: guard
rows around z and zf, rows that are no query, the MLP columns [d, K2) of every
row in both planes, zf rows from zf_rows on, and with zf_last every zf row but
row s; and that the x2f16 range flag is set only where a case says so.  The
inputs carry NaN in every row past a sequence, in the cache's Q columns and in
the Q of rows below q0, so a read of those poisons z.

Bars (attention_cases.bar): 4 x the larger error of two fp32 restatements of
the case, floored at 2^-22 max |V|; ``select`` cases are bit-exact.

Measured on an MI355X by this file (printed at its end), worst max |dz| / bar
over every case of a form: tile NKT 1 0.314 (stage 0, 1 and 2 alike), NKT 2
0.301 (stage 0 and 3), NKT 4 0.305, NKT 8 0.377, chunked 0.294, row kernel
0.212, single-query sequences on the tile kernel 0.351.  Bitwise equal on the
GPU: STAGE 0 / 1 / 2, VSTAGE 0 / 1, a launch and the same sequences padded to
NKT 2 / 4 / 8, zf and z, every format and tvr_act_rows of the fp32 z.  The
whole file (97 tests) runs in about 8 s.  Every forced pattern runs in fp32 and
in the interleaved x2f16 format (``check_il``).

A bug these tests found: the row kernel returned a selected V row 1 ulp off at
d_head 80 and 128 (1 / sqrt(d_head) not a power of two).  ``sc *= scale`` was
contracted into ``expf(sc - m_new)`` as fma(sc, scale, -m_new) while m_new held
the rounded product, so the best key's weight was exp(the product's rounding
error) instead of 1 (read in the disassembly: v_mul_f32 for the max, v_fma_f32
for the exponent).  The product is now rounded once, and the cases are bitwise.

The tests bite: eight mutants of attention_mfma.hpp (not committed), each built
and run once against this file (failing tests of 97): ``key < qpos`` 79; nkq /
kt_end without ``+ 1`` 84; the tile kernel's rotary sign 42; the row kernel's
``sg`` 12; ``min(row, T)`` in the STAGE 3 staging 54; the chunked form without
``zt *= scale`` 60; ``zrow <= zf_rows`` 66; ``zrow + 1 < zf_rows`` 66 (both
kernels, both sides of the zf_rows edge: the rows whose zf copy is due come
from the layout, and each must have been written).
"""
import collections
import functools
import gc
import time

import numpy as np
import pytest
import torch

import attention_cases as A
import tvr_amd

pytestmark = [pytest.mark.gpu]

L = tvr_amd._lib
F32, X2F16, IL, BF16 = 0, L.GEMM_MODES["x2f16"], L.ACT_X2F16_IL, L.GEMM_MODES["bf16"]
FMT_NAME = {F32: "f32", X2F16: "x2f16", IL: "x2f16_il", BF16: "bf16"}
G = 2                    # guard rows before and after every buffer
NAN_BITS = 0x7FC00000    # torch.full(nan)
SENT16 = 0x7FFF
KINDS = ("random", "random_gain", "uniform", "rotary_only", "huge")
ENV = ("TVR_ATT_STAGE", "TVR_ATT_VSTAGE", "TVR_ROW_ATTN")
MODEL_IDS = [f"dh{dh}h{h}" for dh, h in A.MODELS]

_worst = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _module():
    """Times the module, prints the worst ratios, and releases the module's models, cases (with their device
    inputs) and references when its last test is done."""
    t0 = time.time()
    yield
    for form, r in sorted(_worst.items()):
        print(f"\nattention, worst max |dz| / bar: {form:28s} {r:.3f}", end="")
    print(f"\nattention tests: {time.time() - t0:.1f} s from the first test to the last")
    for cache in (_ref, _case, _ctx):
        cache.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


class Ctx:
    def __init__(self, DH, H):
        self.DH, self.H, self.d, self.K2 = DH, H, DH * H, DH * H + A.D_MLP
        cfg = tvr_amd.config.PythiaConfig(1, self.d, H, A.D_MLP, 64, n_ctx=A.N_CTX, name=f"attention-{DH}x{H}")
        w = tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda")
        # no token is ever looked up: any tokenizer (the default one needs a larger vocabulary than 64)
        self.model = tvr_amd.Model(cfg, w, tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda", gemm="f32")
        self.lib, self.h = self.model._lib, self.model._h
        self.cos, self.sin = A.tables(DH)
        self.d_cos, self.d_sin = torch.from_numpy(self.cos).cuda(), torch.from_numpy(self.sin).cuda()
        self.row_kernel = H % (2 if DH == 128 else 4) == 0  # engine.hip row_attention_ok

    def stream(self):
        return self.model._stream()


@functools.lru_cache(maxsize=None)  # one model per (d_head, n_heads) for the module: _module clears it
def _ctx(model):
    return Ctx(*model)


@pytest.fixture(params=A.MODELS, ids=MODEL_IDS)
def ctx(request):
    return _ctx(request.param)


@functools.lru_cache(maxsize=None)
def _case(model, kind, maxT, rows=False, pad=None, rot=0):
    lay = A.batch_rows(maxT) if rows else A.batch(maxT, pad=pad)
    return A.make(kind, model[0], model[1], lay, seed=maxT, rot=rot)


@functools.lru_cache(maxsize=None)
def _ref(model, kind, maxT, rows=False):
    """(case, z64, bar): computed once, shared by every test and form."""
    case = _case(model, kind, maxT, rows)
    c = _ctx(model)
    z64 = A.reference(case, c.cos, c.sin)
    return case, z64, A.bar(case, c.cos, c.sin, z64)[0]


def set_env(monkeypatch, **kv):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv("TVR_" + k, str(v))


def envs_of(maxT):
    """The switches that choose among the forms of a launch whose longest T is maxT."""
    nkt = A.nkt_of(maxT)
    if nkt == 1:
        return [dict(ATT_STAGE=s) for s in (0, 1, 2)]
    if nkt == 2:
        return [dict(ATT_VSTAGE=v) for v in (0, 1)]
    return [{}]


def form_of(ctx, maxT, env):
    nkt = A.nkt_of(maxT)
    if nkt == 0:
        return "tile chunked"
    if nkt == 1:
        st = env.get("ATT_STAGE", 2)
        return f"tile NKT 1 stage {st if ctx.DH <= 80 else 0}"
    if nkt == 2:
        return f"tile NKT 2 stage {3 if env.get('ATT_VSTAGE', 1) else 0}"
    return f"tile NKT {nkt}"


def guarded(a, fill):
    t = torch.full((a.shape[0] + 2 * G,) + tuple(a.shape[1:]), fill, dtype=a.dtype)
    t[G:G + a.shape[0]] = a
    return t.cuda()


def logical(buf, fmt, ld):
    """halves [rows][2 ld] in activation format fmt -> [rows][2 planes][ld] logical columns."""
    rows = buf.shape[0]
    if fmt == IL:
        return buf.reshape(rows, ld // 32, 2, 32).transpose(0, 2, 1, 3).reshape(rows, 2, ld)
    return buf.reshape(rows, 2, ld)


def seq_array(seqs):
    return (L.CAttnSeq * len(seqs))(*[L.CAttnSeq(*s) for s in seqs])


Out = collections.namedtuple("Out", "z planes zf zbuf due")


def launch(ctx, case, fmt=F32, zf=None, tables=True, expect_range=False):
    """One tvr_attention launch on guarded, sentinel-filled buffers.  zf: None, "last" (zf_last) or the
    zf_rows cut.  Returns z [rows][d] fp32 (NaN outside the query rows; fmt 0), planes [rows][2][d] halves
    (other formats), zf [rows][d] (NaN where none was due; zf_last: sequence s' row at its last row) and
    due, the rows whose zf copy the arguments ask for (from the layout, never from the output).
    Asserts that every due zf row was written, that nothing else was, and that the range flag is as expected."""
    lay, d, K2 = case.lay, case.d, ctx.K2
    rows, n = lay.rows, lay.n_seq
    if not hasattr(case, "dev"):  # the inputs go to the device once per case
        case.dev = (guarded(torch.from_numpy(case.qkv), float("nan")), guarded(torch.from_numpy(case.cache), float("nan")))
    qkv, cache = case.dev
    if fmt == F32:
        zbuf = torch.full((rows + 2 * G, K2), float("nan"), dtype=torch.float32, device="cuda")
    else:
        zbuf = torch.full((rows + 2 * G, 2 * K2), SENT16, dtype=torch.int16, device="cuda")
    zf_last, zf_rows, nzf = (1, 0, n) if zf == "last" else (0, 0 if zf is None else int(zf), rows)
    zfbuf = None if zf is None else torch.full((nzf + 2 * G, d), float("nan"), dtype=torch.float32, device="cuda")
    off = lambda t: t.data_ptr() + G * t.stride(0) * t.element_size()
    rc = ctx.lib.tvr_attention(ctx.h, fmt, off(qkv), off(cache), seq_array(lay.seqs), n, lay.row_from, rows,
                               lay.cache_rows, off(zbuf), 0 if zfbuf is None else off(zfbuf), zf_last, zf_rows,
                               ctx.d_cos.data_ptr() if tables else 0, ctx.d_sin.data_ptr() if tables else 0,
                               ctx.stream())
    L.check(rc, "tvr_attention")
    flag = ctx.lib.tvr_model_range_status(ctx.h, ctx.stream())
    assert flag == (L.TVR_ERR_RANGE if expect_range else L.TVR_OK), f"range flag {flag} ({case.kind}, {FMT_NAME[fmt]})"
    q = A.query_rows(lay)
    zh = zbuf.cpu().numpy()
    z = planes = None
    if fmt == F32:
        bits = zh.view(np.int32)
        assert (bits[:G] == NAN_BITS).all() and (bits[-G:] == NAN_BITS).all(), "z guard rows written"
        assert (bits[G:-G][~q] == NAN_BITS).all(), "a row that is no query was written"
        assert (bits[G:-G, d:] == NAN_BITS).all(), "the MLP columns of a2 were written"
        z = zh[G:-G, :d].copy()
    else:
        bits = zh.view(np.uint16)
        assert (bits[:G] == SENT16).all() and (bits[-G:] == SENT16).all(), "z guard rows written"
        lg = logical(bits[G:-G], fmt, K2)
        assert (lg[~q] == SENT16).all(), "a row that is no query was written"
        assert (lg[:, :, d:] == SENT16).all(), "the MLP columns of a2 were written"
        if fmt == BF16:
            assert (lg[:, 1] == SENT16).all(), "bf16 wrote plane 1"
        planes = lg[:, :, :d].copy()
    zfo = due = None
    if zfbuf is not None:
        fh = zfbuf.cpu().numpy()
        fb = fh.view(np.int32)
        assert (fb[:G] == NAN_BITS).all() and (fb[-G:] == NAN_BITS).all(), "zf guard rows written"
        zfo = np.full((rows, d), np.nan, dtype=np.float32)
        if zf == "last":
            due = np.zeros(rows, dtype=bool)
            for s, sd in enumerate(lay.seqs):  # zf has exactly n_seq rows: every one is some sequence's
                zfo[sd.row0 + sd.n - 1] = fh[G + s]
                due[sd.row0 + sd.n - 1] = True
            assert due.sum() == n
        else:
            due = q & (np.arange(rows) < zf_rows)
            assert (fb[G:-G][~due] == NAN_BITS).all(), "a zf row at or past zf_rows, or of no query, was written"
            zfo[due] = fh[G:-G][due]
        assert not np.isnan(zfo[due]).any(), "a zf row that was due was not written (or holds NaN)"
    return Out(z, planes, zfo, zbuf, due)


def zf_cut(lay):
    """A zf_rows that cuts through the queries of a sequence: rows below it are copied, the query row AT it
    and everything above are not.  Single-query launches: the query row of a sequence of the row kernel."""
    if lay.row_from < lay.n_seq:
        sd = lay.seqs[min(lay.row_from + 1, lay.n_seq - 1)]
        return sd.row0 + sd.n - 1
    many = [sd for sd in lay.seqs if sd.n - sd.q0 >= 2]
    sd = many[-1] if many else lay.seqs[-1]
    return sd.row0 + sd.q0 + (sd.n - sd.q0) // 2


def same_bits(a, b, rows):
    return np.array_equal(a[rows].view(np.int32), b[rows].view(np.int32))


def act_rows(ctx, fmt, out32):
    """tvr_act_rows(fmt) of the fp32-format z (device buffer of ``launch``) over columns [0, d) at lda = K2."""
    rows = out32.zbuf.shape[0] - 2 * G
    o = torch.zeros((rows, 2 * ctx.d), dtype=torch.int16, device="cuda")
    L.check(ctx.lib.tvr_act_rows(fmt, out32.zbuf.data_ptr() + G * ctx.K2 * 4, ctx.K2, o.data_ptr(), rows, ctx.d, 0,
                                 ctx.stream()), "tvr_act_rows")
    torch.cuda.synchronize()
    return logical(o.cpu().numpy().view(np.uint16), fmt, ctx.d)


def check_err(ctx, case, z64, bar, out, form, what="z"):
    lay, rf = case.lay, case.lay.row_from
    row_form = "row kernel" if ctx.row_kernel and form[1] else "tile, single query"
    for lo, hi, name in ((0, rf, form[0]), (rf, None, row_form)):
        for arr, label in ((out.z, "z"), (out.zf, "zf")):
            if arr is None:
                continue
            qs = A.query_rows(lay, lo, hi)
            if label == "zf":
                qs &= out.due  # the rows whose copy the launch asked for
            if not qs.any():
                continue
            e = np.abs(arr[qs].astype(np.float64) - z64[qs])
            err = float("inf") if np.isnan(e).any() else float(e.max())
            _worst[name] = max(_worst[name], err / bar)
            print(f"{case.kind} dh {ctx.DH} h {ctx.H} maxT {lay.maxT} {name} {label}: err {err:.3e} bar {bar:.3e} "
                  f"ratio {err / bar:.3f}")
            assert err <= bar, (case.kind, lay.maxT, name, label, err, bar)


def check_il(ctx, case, out32):
    """The same launch in the interleaved x2f16 format (the forced patterns run at fp32 and at it): z is
    tvr_act_rows of the fp32 z bit for bit, zf is the fp32 z on the rows that are due."""
    q = A.query_rows(case.lay)
    p = launch(ctx, case, fmt=IL, zf=zf_cut(case.lay))
    assert np.array_equal(p.planes[q], act_rows(ctx, IL, out32)[q]), (case.kind, case.lay.maxT)
    assert p.due.any() and same_bits(p.zf, out32.z, p.due)


# ---------------------------------------------------------------- 1, 3, 4: accuracy, zf, what is not written
@pytest.mark.parametrize("kind", KINDS)
def test_tile_kernels_against_fp64(ctx, kind, monkeypatch):
    """Every key-tile form and staging form on ragged batches: max |z - z64| <= bar on z and on zf, zf
    bitwise z, under a zf_rows cut and under zf_last."""
    model = (ctx.DH, ctx.H)
    for maxT in A.ALL_T:
        case, z64, bar = _ref(model, kind, maxT)
        q = A.query_rows(case.lay)
        for env in envs_of(maxT):
            set_env(monkeypatch, **env)
            form = (form_of(ctx, maxT, env), False)
            a = launch(ctx, case, zf=zf_cut(case.lay))
            b = launch(ctx, case, zf="last")
            check_err(ctx, case, z64, bar, a, form)
            check_err(ctx, case, z64, bar, b, form)
            assert same_bits(a.z, b.z, q)
            for o in (a, b):
                assert o.due.any() and same_bits(o.zf, o.z, o.due)
            assert a.due.sum() < q.sum()  # the cut leaves query rows out
            check_il(ctx, case, a)


@pytest.mark.parametrize("kind", KINDS)
def test_single_query_launches_against_fp64(ctx, kind, monkeypatch):
    """row_from = 1: the row kernel (TVR_ROW_ATTN 1; the tile kernel where n_heads refuses it) and the
    tile kernel (TVR_ROW_ATTN 0) on the same sequences, each against the reference."""
    model = (ctx.DH, ctx.H)
    for maxT in A.ROW_T:
        case, z64, bar = _ref(model, kind, maxT, True)
        for on in (1, 0):
            set_env(monkeypatch, ROW_ATTN=on)
            form = (form_of(ctx, maxT, {}), bool(on))
            a = launch(ctx, case, zf=zf_cut(case.lay))
            b = launch(ctx, case, zf="last")
            for o in (a, b):
                check_err(ctx, case, z64, bar, o, form)
                assert o.due.any() and same_bits(o.zf, o.z, o.due)
            # the cut is the query row of a single-query sequence: the sequences before it are due, it is not
            assert a.due[A.query_rows(case.lay, 1, 2)].all() and a.due.sum() < A.query_rows(case.lay).sum()
            # and the other side of the edge: the cut one past a single-query sequence's row, which is due
            sd = case.lay.seqs[1]
            c = launch(ctx, case, zf=sd.row0 + sd.n)
            assert c.due[sd.row0 + sd.n - 1] and not c.due[A.query_rows(case.lay, 2)].any()
            assert same_bits(c.zf, c.z, c.due)
            check_il(ctx, case, a)


# ------------------------------------------------------------------------------ 2: exact selection
def test_select_is_bitwise(ctx, monkeypatch):
    """z[i] = V[min(pi[i], i)] bit for bit in the tile (every stage), chunked and row kernels, fp32 and the
    interleaved x2f16 format."""
    model = (ctx.DH, ctx.H)
    fails = []
    for maxT, rows, rot in A.select_launches():
        case = _case(model, "select", maxT, rows, None, rot)
        q = A.query_rows(case.lay)
        want = torch.full((case.lay.rows + 2 * G, ctx.K2), float("nan"))
        want[G:-G, :ctx.d] = torch.from_numpy(case.expect)
        want = act_rows(ctx, IL, Out(None, None, None, want.cuda(), None))
        for env in ([dict(ROW_ATTN=1), dict(ROW_ATTN=0)] if rows else envs_of(maxT)):
            set_env(monkeypatch, **env)
            o = launch(ctx, case, zf="last")
            p = launch(ctx, case, fmt=IL)
            assert same_bits(o.zf, o.z, o.due)
            # per (sequence, head): elements that differ from V[min(pi, i)] and by how many ulp at most
            for s, sd in enumerate(case.seqs):
                for h in range(ctx.H):
                    r, c = slice(sd.row0 + sd.q0, sd.row0 + sd.n), slice(h * ctx.DH, (h + 1) * ctx.DH)
                    a, b = o.z[r, c].view(np.int32).astype(np.int64), case.expect[r, c].view(np.int32).astype(np.int64)
                    pl = (p.planes[r][:, :, c] != want[r][:, :, c]).sum()
                    if (a != b).any() or pl:
                        fam = A.SELECT_FAMILIES[A.select_plan(ctx.DH, ctx.H, s, h, rot)[0]][0]
                        fails.append((maxT, "rows" if rows else "batch", rot, env, f"seq {s} head {h} {fam}",
                                      f"{int((a != b).sum())} of {a.size} differ, {int(np.abs(a - b).max())} ulp; "
                                      f"{int(pl)} halves"))
    for f in fails:
        print("select mismatch:", *f)
    assert not fails, (len(fails), fails[:6])


# ------------------------------------------------------------------------------ 3: formats, range flag
def test_formats_are_act_rows_of_fp32_z(ctx, monkeypatch):
    """x2f16 / interleaved / bf16 z = tvr_act_rows(fmt) of the fp32-format z, bit for bit, in every form."""
    model = (ctx.DH, ctx.H)
    launches = [(t, False, e) for t in A.ALL_T for e in envs_of(t)]
    launches += [(t, True, dict(ROW_ATTN=on)) for t in A.ROW_T for on in (1, 0)]
    for maxT, rows, env in launches:
        case = _case(model, "random", maxT, rows)
        q = A.query_rows(case.lay)
        set_env(monkeypatch, **env)
        o = launch(ctx, case)
        for fmt in (X2F16, IL, BF16):
            p = launch(ctx, case, fmt=fmt, zf=zf_cut(case.lay))
            want = act_rows(ctx, fmt, o)
            npl = 1 if fmt == BF16 else 2
            assert np.array_equal(p.planes[q][:, :npl], want[q][:, :npl]), (maxT, rows, env, FMT_NAME[fmt])
            assert p.due.any() and same_bits(p.zf, o.z, p.due)
            _worst[f"format {FMT_NAME[fmt]}: bitwise act_rows(z)"] = 0.0


def test_range_flag(ctx, monkeypatch):
    """One V row at 5000 reaches z unmixed: the x2f16 formats raise the flag (every store form: staged,
    through LDS, chunked, row kernel); at 4000 (|z| < 4095) and in fp32 / bf16 they do not."""
    model = (ctx.DH, ctx.H)
    for maxT, rows in ((15, False), (17, False), (33, False), (129, False), (15, True)):
        for kind in ("range", "range_below"):
            case = _case(model, kind, maxT, rows)
            set_env(monkeypatch)
            for fmt in (F32, X2F16, IL, BF16):
                launch(ctx, case, fmt=fmt, expect_range=kind == "range" and fmt in (X2F16, IL))
    # the flag of the row kernel alone: the 5000 row belongs to a single-query sequence
    if ctx.row_kernel:
        case = _case(model, "random", 15, True)
        sd = case.lay.seqs[1]
        hot = A.Case("range", ctx.DH, ctx.H, case.lay, case.qkv.copy(), case.cache)
        hot.qkv[sd.row0:sd.row0 + sd.n, 2 * ctx.d:] = 5000.0
        launch(ctx, hot, fmt=IL, expect_range=True)
        launch(ctx, hot, fmt=F32)


# ------------------------------------------------------------------------------ 5: bit-identical forms
def test_key_tile_skipping_is_bit_identical(ctx, monkeypatch):
    """The same sequences in a launch that one longer sequence moves to NKT 2 / 4 / 8 give bitwise the same
    z: a key tile past a query tile's last position is skipped, not computed and masked."""
    model = (ctx.DH, ctx.H)
    for kind in ("random", "random_gain"):
        for maxT, pads in ((1, (32, 64, 128)), (15, (32, 64, 128)), (16, (32, 64, 128)), (17, (64, 128)),
                           (32, (64, 128)), (33, (128,)), (64, (128,))):
            base = _case(model, kind, maxT)
            q = A.query_rows(base.lay)
            set_env(monkeypatch, ATT_STAGE=0, ATT_VSTAGE=0)
            z0 = launch(ctx, base).z
            for pad in pads:
                padded = _case(model, kind, maxT, False, pad)
                assert A.nkt_of(padded.lay.maxT) > A.nkt_of(maxT) and padded.lay.seqs[:-1] == base.lay.seqs
                for env in envs_of(pad):
                    set_env(monkeypatch, **env)
                    z1 = launch(ctx, padded).z[:base.lay.rows]
                    assert same_bits(z1, z0, q), (kind, maxT, pad, env)
    _worst["NKT 1 = 2 = 4 = 8 (key-tile skipping): bitwise"] = 0.0


def test_staging_forms_are_bit_identical(ctx, monkeypatch):
    """TVR_ATT_STAGE 0 / 1 / 2 (one key tile) and TVR_ATT_VSTAGE 0 / 1 (two): the same operands from LDS."""
    model = (ctx.DH, ctx.H)
    for kind in KINDS:
        for maxT in A.MAXT[1] + A.MAXT[2]:
            case = _case(model, kind, maxT)
            q = A.query_rows(case.lay)
            zs = []
            for env in envs_of(maxT):
                set_env(monkeypatch, **env)
                zs.append(launch(ctx, case).z)
            for z in zs[1:]:
                assert same_bits(z, zs[0], q), (kind, maxT)
    _worst["stage 0 = 1 = 2, vstage 0 = 1: bitwise"] = 0.0


# ------------------------------------------------------------------------------ 6: the model's own tables
def test_model_tables(ctx, monkeypatch):
    """cos_t = sin_t = NULL (the tables tvr_model_create computes) against TL's tables on a rotary-only case
    at T = 300.  Bar: twice what moving TL's fp32 frequencies by 2 ulp does to the fp64 reference (the
    engine's powf / division / cosf may each differ from torch's by an ulp), plus the case's bar."""
    model = (ctx.DH, ctx.H)
    set_env(monkeypatch)
    case, z64, bar = _ref(model, "rotary_only", 300)
    f = A.tl_freq32(ctx.DH)
    za = A.reference(case, *A.tables_from_freq(f))
    zb = A.reference(case, *A.tables_from_freq(f * (1 + 2.0 ** -22)))
    shift = A.max_err(zb, za, case.lay)
    own, tl = launch(ctx, case, tables=False).z, launch(ctx, case).z
    diff = A.max_err(own, tl.astype(np.float64), case.lay)
    print(f"model tables dh {ctx.DH}: |z(own) - z(TL)| {diff:.3e}, 2-ulp frequency shift {shift:.3e}, bar {bar:.3e}")
    assert 0 < shift and diff <= 2 * shift + bar
    assert A.max_err(own, z64, case.lay) <= 2 * shift + bar


# ------------------------------------------------------------------------------ 7: validation
def test_invalid_arguments_launch_nothing(monkeypatch):
    """Every TVR_ERR_INVALID of tvr_attention by its message, with nothing written.  Not reachable: the
    interleaved format with K2 % 32 != 0 (tvr_model_create accepts no such model)."""
    ctx = _ctx(A.MODELS[0])
    set_env(monkeypatch)
    case = _case(A.MODELS[0], "random", 33)
    lay, d, K2 = case.lay, case.d, ctx.K2
    qkv, cache = torch.from_numpy(case.qkv).cuda(), torch.from_numpy(case.cache).cuda()
    z = torch.full((lay.rows, K2), float("nan"), device="cuda")
    zf = torch.full((lay.rows, d), float("nan"), device="cuda")
    live = next(i for i, s in enumerate(lay.seqs) if s.prefix_live)
    cached = next(i for i, s in enumerate(lay.seqs) if s.p0 and not s.prefix_live)

    def call(msg, seq=None, **kw):
        seqs = list(lay.seqs)
        if seq:
            i, ch = seq
            seqs[i] = seqs[i]._replace(**ch)
        a = dict(model=ctx.h, fmt=F32, qkv=qkv.data_ptr(), cache=cache.data_ptr(), seqs=seq_array(seqs),
                 n_seq=lay.n_seq, row_from=lay.n_seq, rows=lay.rows, cache_rows=lay.cache_rows, z=z.data_ptr(),
                 zf=zf.data_ptr(), zf_last=0, zf_rows=lay.rows, cos=ctx.d_cos.data_ptr(), sin=ctx.d_sin.data_ptr())
        a.update(kw)
        rc = ctx.lib.tvr_attention(a["model"], a["fmt"], a["qkv"], a["cache"], a["seqs"], a["n_seq"], a["row_from"],
                                   a["rows"], a["cache_rows"], a["z"], a["zf"], a["zf_last"], a["zf_rows"], a["cos"],
                                   a["sin"], ctx.stream())
        err = ctx.lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith("tvr_attention: ") and msg in err, (msg, rc, err)

    call("null model", model=None)
    call("null qkv", qkv=None)
    call("null z", z=None)
    call("null seqs", seqs=None)
    call("n_seq must be positive", n_seq=0)
    call("unknown fmt", fmt=1)
    call("unknown fmt", fmt=0x13)
    call("n must be at least 1", seq=(1, dict(n=0)))
    call("q0 outside [0, n)", seq=(0, dict(q0=-1)))
    call("q0 outside [0, n)", seq=(0, dict(q0=lay.seqs[0].n)))
    call("p0 is negative", seq=(0, dict(p0=-1)))
    call("p0 + n exceeds n_ctx", seq=(cached, dict(p0=A.N_CTX - lay.seqs[cached].n + 1)))
    call("outside the qkv buffer", seq=(0, dict(row0=-1)))
    call("outside the qkv buffer", seq=(lay.n_seq - 1, dict(row0=lay.rows - lay.seqs[-1].n + 1)))
    call("outside the qkv buffer", rows=lay.rows - 2)
    call("cache_row is negative", seq=(cached, dict(cache_row=-1)))
    call("outside the cache buffer", seq=(cached, dict(cache_row=lay.cache_rows - lay.seqs[cached].p0 + 1)))
    call("outside the cache buffer", cache_rows=1)
    call("null cache", cache=None)
    call("outside the qkv buffer", seq=(live, dict(cache_row=lay.rows - lay.seqs[live].p0 + 1)))
    call("prefix_live must be 0 or 1", seq=(live, dict(prefix_live=2)))
    call("needs q0 == n - 1", row_from=0)
    call("row_from outside", row_from=lay.n_seq + 1)
    call("row_from outside", row_from=-1)
    call("rows must be positive", rows=0)
    call("rows must be positive", rows=-3)
    call("cache_rows non-negative", cache_rows=-1)
    call("zf_rows is negative", zf_rows=-1)
    call("both be given or both be null", cos=None)
    call("both be given or both be null", sin=None)
    call("16-byte aligned", qkv=qkv.data_ptr() + 4)
    call("16-byte aligned", z=z.data_ptr() + 8)
    torch.cuda.synchronize()
    assert torch.isnan(z).all() and torch.isnan(zf).all()
    assert ctx.lib.tvr_model_range_status(ctx.h, ctx.stream()) == L.TVR_OK
    # and the unchanged arguments are accepted (the calls above failed for their own reason)
    launch(ctx, case, zf=lay.rows)
