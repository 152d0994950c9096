"""The co-residency guard of the finalize head (csrc/session_mode.cpp fin_head_fits), on the host:
every workgroup of the head launch — n / 64 panels and the publisher — waits for all the others,
so the head is planned only where the device holds them all at once."""


def test_guard_refuses_a_capacity_below_the_grid_and_admits_256_by_2():
    from glx import _lib
    fits = _lib.lib().glx_fin_head_fits
    n = 16384                                # 256 panels + the publisher = 257 workgroups
    assert fits(n, 256, 2) == 1              # MI355X: 256 CUs, two workgroups each
    assert fits(n, 256, 1) == 0              # one short
    assert fits(n, 257, 1) == 1
    assert fits(n, 128, 2) == 0              # a faked capacity below the grid
    assert fits(n, 0, 2) == 0 and fits(n, 256, 0) == 0   # an occupancy query that failed
    assert fits(64, 1, 2) == 1 and fits(64, 1, 1) == 0   # one panel + the publisher
    assert fits(64 * 1023, 256, 2) == 0      # the largest fused grid (1024 workgroups) on 512 slots
    assert fits(64 * 511, 256, 2) == 1 and fits(64 * 512, 256, 2) == 0
