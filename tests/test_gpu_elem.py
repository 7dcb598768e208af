"""Small device kernels of the input side (csrc/elem.hip) against their torch statements, and every element of the pack / unpack / max-pool /
sine-position kernels against the references of tests/row_bounds.py."""
import pytest
import torch

import row_bounds as rw
from rounding_bounds import BF, F32

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture
def dev():
    return torch.device("cuda")


def test_text_prep_matches_the_hf_position_ids_and_the_padding_mask(dev):
    """toist_text_prep: RoBERTa's create_position_ids_from_input_ids (cumsum(id != pad) * (id != pad) + pad) and attention_mask != 1
    (/root/reference/models/transformer.py:129-133 through HF RobertaModel) in one launch; ragged captions, a pad id inside a caption."""
    from toist_amd import kernels as k
    torch.manual_seed(0)
    for B, L in ((1, 1), (3, 7), (8, 16), (70, 33)):
        ids = torch.randint(3, 500, (B, L), device=dev)
        lens = torch.randint(1, L + 1, (B,), device=dev)
        att = (torch.arange(L, device=dev)[None, :] < lens[:, None]).long()
        ids = torch.where(att.bool(), ids, torch.ones_like(ids))               # <pad> = 1 behind every caption
        if L > 3:
            ids[0, 1] = 1                                                        # a pad id in the middle (counts as padding for the positions)
        pos, key_pad = k.text_prep(ids, att, 1)
        keep = ids.ne(1).long()
        assert torch.equal(pos, torch.cumsum(keep, dim=1) * keep + 1)
        assert torch.equal(key_pad, att.ne(1).to(torch.uint8))


def test_sine_position_seq_is_the_token_encoding_with_zero_caption_rows(dev):
    """toist_sine_position_seq writes PositionEmbeddingSine's token-major rows straight into the cross-modal sequence layout [B, H*W + L, 256];
    the L caption rows are zero (transformer.py:139); the image rows equal toist_sine_position's bit for bit."""
    from toist_amd.position_encoding import PositionEmbeddingSine
    pe = PositionEmbeddingSine(128, normalize=True)
    torch.manual_seed(1)
    for B, H, W, L in ((2, 5, 7, 3), (8, 20, 20, 16), (1, 1, 1, 1)):
        mask = torch.rand(B, H, W, device=dev) > 0.7
        mask[:, 0, 0] = False
        plain = pe.tokens(mask)
        seq = pe.tokens(mask, tail=L)
        assert seq.shape == (B, H * W + L, 256)
        assert torch.equal(seq[:, :H * W], plain)
        assert not seq[:, H * W:].any()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Every element of the pack / unpack / max-pool / sine-position kernels against tests/row_bounds.py: bit for bit where the kernel only moves or
# rounds values, within the derived bound for the sine encoding; outputs start as NaN, grids above their 4096-block cap stride.
@pytest.mark.parametrize("C", rw.PACK_C)
def test_pack_image_every_element(dev, C):
    from toist_amd import kernels as k
    for N, H, W in rw.PACK_NHW:
        x = rw.pack_inputs(N, C, H, W)
        out = torch.full((N, H, W, 8), NAN, dtype=BF, device=dev)
        k.pack_image(x.to(dev), out)
        rw.check_exact("pack_image", f"{N}x{C}x{H}x{W}", out, rw.pack_ref(x))


def test_pack_image_grid_strides(dev):
    from toist_amd import kernels as k
    N, C, H, W = rw.PACK_BIG
    x = rw.pack_inputs(N, C, H, W)
    out = torch.full((N, H, W, 8), NAN, dtype=BF, device=dev)
    k.pack_image(x.to(dev), out)
    rw.check_exact("pack_image", f"{N}x{C}x{H}x{W}", out, rw.pack_ref(x))


@pytest.mark.parametrize("N,HW,C", rw.UNPACK)
def test_unpack_nhwc_every_element(dev, N, HW, C):
    from toist_amd import kernels as k
    x = rw.unpack_inputs(N, HW, C)
    out = torch.full((N, C, HW), NAN, dtype=F32, device=dev)
    k.unpack_nhwc(x.to(dev), out)
    rw.check_exact("unpack_nhwc", f"{N}x{HW}x{C}", out, rw.unpack_ref(x))


def _maxpool(dev, x, case):
    from toist_amd import kernels as k
    N, H, W, C = x.shape
    out = torch.full((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), NAN, dtype=BF, device=dev)
    k.maxpool3x3s2(x.to(dev), out)
    rw.check_exact("maxpool3x3s2", case, out, rw.maxpool_ref(x))


@pytest.mark.parametrize("C", rw.POOL_C)
def test_maxpool_every_element(dev, C):
    for N, H, W in rw.POOL_NHW:
        x = rw.pool_inputs(N, H, W, C)
        _maxpool(dev, x, f"{N}x{H}x{W}x{C}")
    x = rw.pool_inputs(2, 7, 9, C, negative=True)      # all negative: a 0 from the padding would win
    _maxpool(dev, x, f"2x7x9x{C} all negative")


def test_maxpool_grid_strides(dev):
    N, H, W, C = rw.POOL_BIG
    x = rw.pool_inputs(N, H, W, C)
    _maxpool(dev, x, f"{N}x{H}x{W}x{C}")


def _sine_case(dev, B, H, W, kind):
    """both outputs at once, each alone (bit-equal to the joint call), and the sequence form with a tail of 0 and of 16 rows"""
    from toist_amd import kernels as k
    mask = rw.sine_mask(B, H, W, kind)
    m8 = mask.to(torch.uint8).to(dev)
    case = f"{B}x{H}x{W} mask={kind}"
    F2 = 2 * rw.SINE_F
    tok = torch.full((B, H * W, F2), NAN, dtype=BF, device=dev)
    nchw = torch.full((B, F2, H, W), NAN, dtype=F32, device=dev)
    k.sine_position(m8, rw.SINE_F, rw.SINE_T, out_tok=tok, out_nchw=nchw)
    ref, bound = rw.sine_nchw_ref(mask)
    measured = float((nchw.cpu().double() - ref).abs().max())
    r = rw.record("sine_position.nchw", case, rw.rb.ratio(nchw, ref, bound), extra={"measured_sine_abs_err": measured, "sine_lib_term": rw.SINE_LIB})
    tref, tbound = rw.sine_tok_ref(mask)
    rw.check("sine_position.tokens", case, tok, tref, tbound)
    assert r <= 1.0, f"sine_position.nchw [{case}]: max err/bound {r} (measured abs err {measured})"
    tok1 = torch.full_like(tok, NAN)
    k.sine_position(m8, rw.SINE_F, rw.SINE_T, out_tok=tok1)
    nchw1 = torch.full_like(nchw, NAN)
    k.sine_position(m8, rw.SINE_F, rw.SINE_T, out_nchw=nchw1)
    rw.check_exact("sine_position.tokens alone", case, tok1, tok)
    rw.check_exact("sine_position.nchw alone", case, nchw1, nchw)
    for tail in (0, 16):
        seq = torch.full((B, H * W + tail, F2), NAN, dtype=BF, device=dev)
        k.sine_position_seq(m8, rw.SINE_F, rw.SINE_T, seq)
        rw.check("sine_position_seq", f"{case} tail={tail}", seq, *rw.sine_tok_ref(mask, tail))


@pytest.mark.parametrize("B,H,W", rw.SINE_BHW)
def test_sine_position_against_the_formula(dev, B, H, W):
    for kind in rw.SINE_MASKS:
        _sine_case(dev, B, H, W, kind)


def test_sine_position_grid_strides(dev):
    _sine_case(dev, *rw.SINE_BIG, "random")
