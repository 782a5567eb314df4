"""Model of the cluster image and the markers' colours (include/mod_sf.h ModClusterImage), written from the
stated arithmetic alone: the built-in table, the index rule (k * 255) // K, and the renderer with black outside [0, K)."""
import numpy as np


def palette() -> np.ndarray:
    """The built-in table, (256, 3) uint8 as B, G, R."""
    lut = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        t = 6 * i
        s, f = t >> 8, t & 255
        g = 255 - f
        r, gg, b = [(255, f, 0), (g, 255, 0), (0, 255, f), (0, g, 255), (f, 0, 255), (255, 0, g)][s]
        lut[i] = (b, gg, r)
    return lut


def index(k: int, K: int) -> int:
    """Table entry of label k among K clusters, 0 <= k < K (ColorSet::resize: i * 255 / n, integer division)."""
    return (int(k) * 255) // int(K)


def render(labels, K_per_frame, lut=None) -> np.ndarray:
    """labels (F, ...) int32, K_per_frame (F,) -> (F, ..., 3) uint8: lut[index(label, K)] inside [0, K), black elsewhere.
    K <= 0 renders black and divides nothing."""
    lut = palette() if lut is None else np.asarray(lut, dtype=np.uint8).reshape(256, 3)
    labels = np.asarray(labels)
    out = np.zeros(labels.shape + (3,), dtype=np.uint8)
    for f, K in enumerate(np.asarray(K_per_frame).reshape(-1)):
        K = int(K)
        if K <= 0:
            continue
        lab = labels[f].astype(np.int64)
        inside = (lab >= 0) & (lab < K)
        idx = np.where(inside, lab * 255 // K, 0)
        out[f] = np.where(inside[..., None], lut[idx], 0)
    return out
