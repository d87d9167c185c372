"""wino.hip's geometry refuses sequences of 2 GiB and more (no GPU needed).

The patch DMA addresses a sequence through a buffer descriptor: 32-bit byte offsets per lane, num_records = the sequence's byte
size, and 0x80000000 as the offset of a padding lane — which is only out of range, for every channel slice and without wrapping,
while every valid offset is below it: T x F x 128 channels x 4 bytes < 2^31, T x F < 2^22.  Past the limit the shape reports 0
rows and the plan keeps the direct kernels."""


def test_winograd_geometry_refuses_sequences_of_2_gib():
    from sed_crnn_amd import _lib
    L = _lib.lib()
    F = 64                                                    # whole tile rows of 32 tiles, two per block
    assert 65536 * F * 128 * 4 == 1 << 31
    assert L.sed_conv3x3_wino_rows(1, 128, F, 65536, 64) == 0             # exactly 2 GiB: the last valid offsets would end at the sentinel
    assert L.sed_conv3x3_wino_rows(1, 128, F, 65538, 64) == 0
    assert L.sed_conv3x3_wino_rows(1, 128, F, 65534, 64) == -(-65534 * F // 4 // 64)     # one tile row below: taken (ceil(tiles / 64) blocks)
    assert L.sed_conv3x3_wino_rg_rows(1, 128, F, 65536, 128, 1) == 0
    # the limit is per sequence, not per batch
    assert L.sed_conv3x3_wino_rows(4, 128, F, 16384, 64) == 4 * 16384 * F // 4 // 64
