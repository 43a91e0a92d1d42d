"""The guard-band helpers of tests/util.py on CPU tensors: a stray byte on either side of a guarded view is found and
located, a moated operand is its source, and the view sits where an allocation would."""
import pytest
import torch

from util import GUARD_BYTES, guarded, guards_intact, moated

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.uint8, torch.float64]


@pytest.mark.parametrize('tdt', DTYPES)
@pytest.mark.parametrize('shape', [(3, 5, 7), (1,), (2, 0, 4), (513,)])
def test_guarded_layout(tdt, shape):
    buf, view = guarded(shape, tdt, 'cpu')
    nbytes = view.numel() * view.element_size()
    assert tuple(view.shape) == shape and view.dtype == tdt and view.is_contiguous()
    off = view.storage_offset() * view.element_size() - buf.storage_offset()
    assert off == GUARD_BYTES and off % 512 == 0 and buf.data_ptr() % 512 == 0
    if nbytes:                                                          # (an empty view, a zero-byte workspace, has no address)
        assert view.data_ptr() == buf.data_ptr() + off
    assert buf.dtype == torch.uint8 and buf.numel() == 2 * GUARD_BYTES + nbytes
    assert bool((buf == 0xFF).all())                                    # guards and the view's own bytes
    if tdt.is_floating_point:
        assert bool(torch.isnan(view).all())                            # ... which read as NaN
    elif tdt != torch.uint8:
        assert bool((view == -1).all())                                 # ... or as -1
    assert guards_intact(buf, view)
    view.zero_()                                                        # writing the whole view leaves the guards alone
    assert guards_intact(buf, view)


def test_one_byte_before_and_behind_is_located():
    buf, view = guarded((4, 6), torch.float32, 'cpu')
    nbytes = 4 * 6 * 4
    buf[GUARD_BYTES - 1] = 0                                            # the byte just before the view
    with pytest.raises(AssertionError, match=r'before .* offset -1 from the view \(1 changed\)'):
        guards_intact(buf, view)
    buf[GUARD_BYTES - 1] = 0xFF
    buf[GUARD_BYTES + nbytes] = 0xFE                                    # the byte just behind it
    with pytest.raises(AssertionError, match=r'behind .* offset %d from the view \(1 changed\)' % nbytes):
        guards_intact(buf, view)
    buf[GUARD_BYTES + nbytes] = 0xFF
    buf[0] = 1                                                          # the far ends belong to the guards too
    with pytest.raises(AssertionError, match=r'offset -%d from' % GUARD_BYTES):
        guards_intact(buf, view)
    buf[0] = 0xFF
    buf[-1] = 1
    with pytest.raises(AssertionError, match=r'offset %d from' % (nbytes + GUARD_BYTES - 1)):
        guards_intact(buf, view)
    buf[-1] = 0xFF
    buf[GUARD_BYTES + nbytes + 7] = 0                                   # of several changed bytes the first is named
    buf[GUARD_BYTES + nbytes + 900] = 0
    with pytest.raises(AssertionError, match=r'offset %d from the view \(2 changed\)' % (nbytes + 7)):
        guards_intact(buf, view)


def test_a_view_one_row_short_catches_the_full_write():
    """What a kernel overrunning its output does: the full shape written through a view that is one row short."""
    buf, view = guarded((4, 6), torch.bfloat16, 'cpu')
    full = torch.ones((5, 6), dtype=torch.bfloat16)
    torch.as_strided(view, (5, 6), (6, 1)).copy_(full)
    with pytest.raises(AssertionError, match=r'behind .* offset %d from the view \(12 changed\)' % (4 * 6 * 2)):
        guards_intact(buf, view)


def test_guards_intact_refuses_foreign_pairs():
    buf, view = guarded((8,), torch.float32, 'cpu')
    with pytest.raises(AssertionError, match='not a guarded'):
        guards_intact(buf, view[1:])
    with pytest.raises(AssertionError, match='not a guarded'):
        guards_intact(buf[1:], view)


@pytest.mark.parametrize('tdt', DTYPES)
def test_moated_operand_equals_its_source(tdt):
    g = torch.Generator().manual_seed(3)
    src = (torch.randn((2, 3, 5, 4), generator=g) * 40).to(tdt)
    m = moated(src)
    assert m.dtype == src.dtype and m.shape == src.shape and m.data_ptr() != src.data_ptr() and m.data_ptr() % 512 == 0
    assert torch.equal(m, src)
    # what lies around it is the poison
    raw = m.untyped_storage()
    lead = m.data_ptr() - raw.data_ptr()
    flat = torch.empty(0, dtype=torch.uint8).set_(raw)
    nbytes = m.numel() * m.element_size()
    assert lead >= GUARD_BYTES and flat.numel() - lead - nbytes >= GUARD_BYTES
    assert bool((flat[lead - GUARD_BYTES:lead] == 0xFF).all()) and bool((flat[lead + nbytes:lead + nbytes + GUARD_BYTES] == 0xFF).all())


@pytest.mark.parametrize('tdt', [torch.float32, torch.bfloat16, torch.uint8])
def test_islands_layout_and_bands(tdt):
    """Islands: regions `step` bytes apart in a buffer that is never filled as a whole; each region reads as the poison, the strided
    view addresses region i as [i], and a byte written in any band -- not between the bands -- is found and located."""
    from util import Islands
    es = torch.empty((), dtype=tdt).element_size()
    shape, n, step = (3, 5, 8), 3, 5 * GUARD_BYTES + 4096
    used = 3 * 5 * 8 * es
    isl = Islands(n, used, step, 'cpu')
    assert isl.buf.dtype == torch.uint8 and isl.buf.numel() == (n - 1) * step + used + 2 * GUARD_BYTES and isl.buf.data_ptr() % 512 == 0
    v = isl.view(shape, tdt)
    assert tuple(v.shape) == (n,) + shape and v.dtype == tdt and v.stride(0) * es == step and v[1].is_contiguous()
    assert v.data_ptr() == isl.data_ptr() == isl.buf.data_ptr() + GUARD_BYTES
    for i in range(n):
        assert v[i].data_ptr() == isl.data_ptr() + i * step == isl.region(i).data_ptr()
        assert bool((isl.region(i) == 0xFF).all())
        if tdt.is_floating_point:
            assert bool(torch.isnan(v[i]).all())
    assert isl.intact()
    v.zero_()                                                           # writing every region leaves the bands alone
    assert isl.intact() and bool((isl.region(2) == 0).all())
    isl.buf[step + 3 * GUARD_BYTES] = 0x12                              # between the bands of regions 1 and 2: nobody's
    assert isl.intact()
    isl.buf[step + GUARD_BYTES - 1] = 0                                 # the byte just before region 1
    with pytest.raises(AssertionError, match=r'before region 1 .* offset -1 from the region \(1 changed\)'):
        isl.intact()
    isl.buf[step + GUARD_BYTES - 1] = 0xFF
    isl.buf[2 * step + GUARD_BYTES + used] = 0                          # the byte just behind region 2, and the last one of its band
    isl.buf[-1] = 0
    with pytest.raises(AssertionError, match=r'behind region 2 .* offset %d from the region \(2 changed\)' % used):
        isl.intact()
    isl.buf[2 * step + GUARD_BYTES + used] = 0xFF
    with pytest.raises(AssertionError, match=r'behind region 2 .* offset %d from' % (used + GUARD_BYTES - 1)):
        isl.intact()
    isl.buf[-1] = 0xFF
    isl.buf[0] = 7                                                      # the first byte of the first band
    with pytest.raises(AssertionError, match=r'before region 0 .* offset -%d from' % GUARD_BYTES):
        isl.intact()


def test_islands_refuses_overlapping_regions():
    from util import Islands
    with pytest.raises(AssertionError):
        Islands(2, 4096, 4096 + GUARD_BYTES, 'cpu')                     # (the bands of neighbours would share bytes with a region)
    with pytest.raises(AssertionError):
        Islands(2, 4096, 4 * GUARD_BYTES + 8, 'cpu')                    # (steps are whole 16-byte units)


def test_prior_contents_for_accumulating_outputs():
    prior = torch.arange(12, dtype=torch.float32).view(3, 4)
    buf, view = guarded((3, 4), torch.float32, 'cpu', prior=prior)
    assert torch.equal(view, prior) and guards_intact(buf, view)
