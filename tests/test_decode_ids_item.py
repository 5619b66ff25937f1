"""CPU: engine.check_decode_ids_item, the preconditions piece.decode_chunks_id_checked raises before
any hashing or device work: check_decode_check_item's, in its order, then the ids'."""

import pytest

from storb_amd import _lib
from storb_amd.engine import Error, check_decode_ids_item

B2 = [b"ab"] * 6
I6 = [bytes(20)] * 6


@pytest.mark.parametrize("item,code", [
    ((4, 6, B2, [0, 1, 2, 3, 4], 0, I6), _lib.SEC_ENBLOCKS),            # blocks and sharenums differ in number
    ((4, 6, [b"ab"] * 5 + [b"abc"], [0, 1, 2, 3, 4, 5], 0, I6), _lib.SEC_EBLOCKLEN),
    ((0, 6, B2, [0, 1, 2, 3, 4, 5], 0, I6), _lib.SEC_EKM),
    ((7, 6, B2, [0, 1, 2, 3, 4, 5], 0, I6), _lib.SEC_EKM),
    ((4, 257, B2, [0, 1, 2, 3, 4, 5], 0, I6), _lib.SEC_EKM),
    ((4, 6, B2[:3], [0, 1, 2], 0, I6[:3]), _lib.SEC_ENBLOCKS),          # n < k
    ((4, 5, B2, [0, 1, 2, 3, 4, 5], 0, I6), _lib.SEC_ENBLOCKS),         # n > m
    ((4, 6, B2, [0, 1, 2, 3, 4, 6], 0, I6), _lib.SEC_ESHARENUM),
    ((4, 6, B2, [0, 1, 2, 3, 4, -1], 0, I6), _lib.SEC_ESHARENUM),
    ((4, 6, B2, [0, 1, 2, 3, 4, 4], 0, I6), _lib.SEC_EDUPSHARE),
    ((4, 6, B2, [0, 1, 2, 2, 4, 5], 0, I6), _lib.SEC_EDUPSHARE),
    ((4, 6, B2, [0, 1, 2, 3, 4, 5], -1, I6), _lib.SEC_EPADLEN),
    ((4, 6, B2, [0, 1, 2, 3, 4, 5], 9, I6), _lib.SEC_EPADLEN),          # padlen > k*B
    ((4, 6, B2, [0, 1, 2, 3, 4, 4], 0, I6[:5]), _lib.SEC_EDUPSHARE),    # the decode + check's own come first
])
def test_item_preconditions_raise_without_a_device(item, code):
    with pytest.raises(Error) as e:
        check_decode_ids_item(*item)
    assert str(e.value) == _lib.strerror(code)


@pytest.mark.parametrize("ids", [I6[:5], I6 + I6[:1], [], I6[:5] + [bytes(19)], [bytes(21)] + I6[1:]])
def test_wrong_id_count_and_wrong_id_length(ids):
    with pytest.raises(ValueError):
        check_decode_ids_item(4, 6, B2, [0, 1, 2, 3, 4, 5], 0, ids)


def test_valid_items_pass():
    check_decode_ids_item(4, 6, B2, [5, 0, 3, 2, 4, 1], 8, I6)
    check_decode_ids_item(4, 6, B2[:4], [5, 0, 3, 2], 0, I6[:4])  # n == k: fully checked all the same
