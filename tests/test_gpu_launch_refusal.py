"""The LDS refusal of the checked launch (csrc/launch.h): a kernel that would need more than a CU's 160 KiB of LDS is
refused with HNSW_ERR_ARG and the launch site's own text before anything is launched.  The one site an input can bring
there is the insert kernel's."""
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib

pytestmark = pytest.mark.gpu

# An index's first SEED = 2048 points are inserted on the host, one after the other, and only what is left of a bulk goes
# to the device (device_build.cpp, gpu_insert_bulk_full: `take = n_before < SEED ? min(order.size(), SEED - n_before) : 0`,
# and nothing goes to the device when `take` is all there is).  On an empty index the smallest bulk that enters a device
# batch has 2049 points; at this shape the sequential seed alone takes half a minute of host time, so the index is
# brought to SEED points by the host build on all threads first, and the smallest device bulk is then ONE point.
SEED = 2048


def test_insert_kernel_that_needs_too_much_lds_is_refused_before_launch():
    """f32, d = 4096, m = 64, ef_construction = 160: layer-0 rows of S0 = 128 slots (> 64), and 160 * 128 / 32 = 640
    > 576 asks for the 2^15-slot visited table (launch_insert, default_slots_log2).  LDS = 131072 (table) + 4096
    (merge buffer) + 1024 (selected keys) + 2 * 16384 (the staged point, twice) + 256 (rank words) = 169216 bytes
    > 163840.  No check of device_build.cpp refuses the shape earlier (m <= 128, ef_construction <= 512, ids far
    below 2^30, a handful of layers): the first batch's launch_insert does, before anything is launched."""
    m, ef_cons, d = 64, 160, 4096
    vs = H.synth_rows(0, 0x1D5, 0, SEED + 1, d)
    idx = H.HNSW.new(m, ef_cons, d, H.VEC_F32).insert_bulk(vs[:SEED], 16, False)
    idx.set_option("gpu_build", 2)  # the device-connect build
    with pytest.raises(_lib.HnswError) as err:
        idx.insert_bulk(vs[SEED:], 8, False)  # n_before = SEED: no host seed, one device batch of one point
    assert err.value.code == _lib.ERR_ARG
    assert "insert kernel needs 169216 bytes of LDS" in str(err.value)
    assert b"insert kernel needs 169216 bytes of LDS" in _lib.lib().hnsw_last_error()
    # the handle is still a handle: it answers, and it can be freed
    assert idx.len() == SEED + 1
    idx.__del__()
    assert idx._h is None
