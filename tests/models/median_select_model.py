"""k_median's bin search in plain Python: which rounds a cluster's norms take before the median member is ranked.

The kernel looks for the member at position size / 2 of the norms sorted descending.  Norms are >= 0 and never NaN, so their F32
bit patterns order like the values.  Each round spreads the live range [lo, hi] over 2048 bins of 2^shift patterns, finds the bin
that holds the rank, and narrows the range to it.  A round with shift == 0 ends the search (`exact`: one value per bin, all its
members tie); so does a bin with at most K_MED_DIRECT members (they are ranked directly in LDS).

A round takes 11 bits off a range of at most 31 bits (norms never have the sign bit): the shifts are at most 20, 9 and 0, so a
third round is always exact and a search that ends in direct ranking has at most two rounds (test_median_select_model.py).
"""
import numpy as np

K_MED_BINS = 2048
K_MED_DIRECT = 256


def shift_of(rng):
    return 0 if rng < K_MED_BINS else int(rng).bit_length() - 11


def select(bits):
    """bits: uint32 norm patterns of one cluster's members.  Returns (rounds, exact, value, nties): rounds is a list of dicts
    (range, shift, bin, inbin = members in the rank's bin, rem = rank inside it); value / nties the median's pattern and how many
    members have it."""
    bits = np.asarray(bits, np.uint32).astype(np.int64)
    lo, hi, rem = int(bits.min()), int(bits.max()), bits.size // 2
    rounds, exact = [], False
    for _ in range(8):
        rng = hi - lo
        shift = shift_of(rng)
        live = bits[(bits >= lo) & (bits <= hi)]
        cnt = np.bincount((live - lo) >> shift, minlength=K_MED_BINS)
        assert cnt.size == K_MED_BINS
        above = np.cumsum(cnt[::-1])                         # members in the bins from the top down to and including bin 2047 - i
        i = int(np.searchsorted(above, rem, side="right"))   # first bin (from the top) whose running count exceeds rem
        b = K_MED_BINS - 1 - i
        rem -= int(above[i] - cnt[b])
        nlo = lo + (b << shift)
        nhi = nlo + (1 << shift) - 1 if shift else nlo
        lo, hi = nlo, min(nhi, hi)
        rounds.append({"range": rng, "shift": shift, "bin": b, "inbin": int(cnt[b]), "rem": rem})
        if shift == 0:
            exact = True
            break
        if cnt[b] <= K_MED_DIRECT:
            break
    value = int(np.sort(bits)[::-1][bits.size // 2])
    assert lo <= value <= hi
    return rounds, exact, value, int((bits == value).sum())
