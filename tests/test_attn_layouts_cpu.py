"""The layouts the attention kernels cannot serve are HOST errors (QS_EINVAL), raised in front of every device call - so these
run without a GPU, on made-up non-null addresses, and no kernel is ever launched on a bad layout.  include/qserve_amd.h states the
contract these pin; tests/test_attn_layouts_gpu.py covers everything it accepts."""
EINVAL = -1
A = 0x10000           # a made-up 256-byte aligned "address"


def test_flash_entry_refuses_layouts_it_cannot_serve(built_lib):
    from qserve_amd._lib import lib
    H, Hkv = 8, 2

    def call(q=A, k=2 * A, v=3 * A, out=4 * A, qs=H * 128, ks=Hkv * 128, vs=Hkv * 128, os_=H * 128, batch=1, msq=4):
        return lib.qs_flash_attn_varlen_fwd(q, k, v, out, 5 * A, 6 * A, batch, H, Hkv, 128, qs, ks, vs, os_, msq, 4, 0.088, 1, None)

    def refused(word, **kw):
        return call(**kw) == EINVAL and word in lib.qs_last_error()

    assert call(batch=0) == 0 and call(msq=0) == 0                      # accepted, empty: returns before any device call
    # base alignment: q / k / v 16 bytes, out 8 bytes
    for name in ("q", "k", "v"):
        assert refused(b"aligned", **{name: A + 8}) and refused(b"aligned", **{name: A + 2})
    assert refused(b"aligned", out=4 * A + 4) and refused(b"aligned", out=4 * A + 2)
    assert call(out=4 * A + 8, batch=0) == 0                            # out 8- but not 16-byte aligned is served (8-byte stores)
    # strides: multiples of 8 elements (out: 4), at least the token's heads, below 2^24
    for name, width in (("qs", H * 128), ("ks", Hkv * 128), ("vs", Hkv * 128)):
        assert refused(b"16-byte", **{name: width + 4}) and refused(b"shorter", **{name: width - 8}) and refused(b"shorter", **{name: 0})
        assert refused(b"2^24", **{name: 1 << 24}) and refused(b"shorter", **{name: -width})
        assert call(**{name: width + 8}, batch=0) == 0 and call(**{name: (1 << 24) - 8}, batch=0) == 0
    assert refused(b"16-byte", os_=H * 128 + 2) and refused(b"shorter", os_=H * 128 - 4) and refused(b"2^24", os_=1 << 24)
    assert call(os_=H * 128 + 4, batch=0) == 0


def test_append_entry_refuses_layouts_it_cannot_serve(built_lib):
    from qserve_amd._lib import lib
    H, Hkv, W = 8, 2, 12 * 128

    def call(qkv=A, out=2 * A, qs=W, os_=H * 128, T=4):
        return lib.qs_append_attention(qkv, out, 3 * A, 4 * A, 5 * A, T, 1, 4, 2, H, Hkv, 128, qs, os_, 64, Hkv * 64, 1, 1, None)

    assert call(T=0) == 0                                               # accepted, empty
    assert call(qkv=A + 8) == EINVAL and call(out=2 * A + 8) == EINVAL  # 16-byte aligned bases
    assert call(qs=W + 4) == EINVAL and call(qs=W - 8) == EINVAL and call(qs=1 << 24) == EINVAL
    assert call(os_=H * 128 + 4) == EINVAL and call(os_=H * 128 - 8) == EINVAL
    assert call(qs=W + 8, os_=H * 128 + 8, T=0) == 0 and call(qs=(1 << 24) - 8, T=0) == 0


def test_decode_entries_refuse_layouts_they_cannot_serve(built_lib):
    from qserve_amd._lib import lib
    H, Hkv = 8, 2

    def call(q=A, k=2 * A, v=3 * A, out=4 * A, qs=H * 128, kvs=Hkv * 128, batch=0, quant=False):
        tail = (batch, H, Hkv, 128, qs, kvs, 2, 8192, 64, Hkv * 64, 10, 128, 1e4, 1, 1, 1, None)
        if quant:
            return lib.qs_single_query_attention_quant(q, k, v, 5 * A, 6 * A, out, 7 * A, 0, 8 * A, *tail)
        return lib.qs_single_query_attention(q, k, v, 5 * A, 6 * A, out, *tail)

    for quant in (False, True):
        assert call(quant=quant) == 0                                   # accepted (batch 0: returns before any device call)
        assert call(qs=H * 128 + 8, kvs=Hkv * 128 + 40, quant=quant) == 0
        for batch in (0, 3):                                            # refused whatever the batch: the checks come first
            for name in ("q", "k", "v", "out"):
                assert call(**{name: A + 8}, batch=batch, quant=quant) == EINVAL and b"aligned" in lib.qs_last_error()
            assert call(qs=H * 128 + 4, batch=batch, quant=quant) == EINVAL and call(kvs=Hkv * 128 + 4, batch=batch, quant=quant) == EINVAL
            assert call(qs=H * 128 - 8, batch=batch, quant=quant) == EINVAL and call(kvs=Hkv * 128 - 8, batch=batch, quant=quant) == EINVAL
            assert call(qs=0, batch=batch, quant=quant) == EINVAL and b"strides" in lib.qs_last_error()

