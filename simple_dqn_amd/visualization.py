"""Filter visualisation page — the reference's --visualization_file (src/main.py:119-127 -> src/visualization.py, which runs Neon's
DeconvCallback and writes an HTML summary page).

The arithmetic runs in libsdqn_hip (DeepQNetwork.visualize: maximum-activation search + guided backpropagation on the device); this
module turns the records into a self-contained HTML page: one block per conv layer, one entry per feature map with the projection and
the winning input state, each an inline PNG written with the standard library only (zlib, struct, base64).
"""
import base64
import html
import logging
import struct
import zlib

import numpy as np

logger = logging.getLogger(__name__)

LAYERS = (("Layer 0000", "conv1"), ("Layer 0002", "conv2"), ("Layer 0004", "conv3"))   # Neon's layer indexes of the three convolutions


def png_bytes(img):
    """uint8 [H, W] (grey) or [H, W, 3] (RGB) -> PNG file bytes: 8-bit samples, filter 0 on every row, one zlib stream."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    if a.ndim == 2:
        color = 0
    elif a.ndim == 3 and a.shape[2] == 3:
        color = 2
    else:
        raise ValueError("expected [H, W] or [H, W, 3], got %s" % (a.shape,))
    h, w = a.shape[:2]
    rows = a.reshape(h, -1)
    raw = b"".join(b"\x00" + rows[y].tobytes() for y in range(h))

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b""))


def png_data_uri(img):
    return "data:image/png;base64," + base64.b64encode(png_bytes(img)).decode("ascii")


def encode_projection(vis):
    """float [4, 84, 84] -> uint8 RGB [84, 84, 3]: taken as HWC, the whole array min-max scaled to [0, 255] (left as it is when its
    range is 0), truncated to uint8; the image shows channels 1, 2, 3 (the oldest frame is dropped)."""
    x = np.transpose(np.asarray(vis, dtype=np.float32), (1, 2, 0))
    lo, hi = float(x.min()), float(x.max())
    if hi > lo:
        x = (x - lo) * (255.0 / (hi - lo))
    return x.astype(np.uint8)[:, :, 1:4]


def encode_state(state):
    """u8 [4, 84, 84] -> the input panel: channels 1, 2, 3 as RGB, unscaled."""
    return np.ascontiguousarray(np.transpose(np.asarray(state, dtype=np.uint8), (1, 2, 0))[:, :, 1:4])


def summary_page(layers, state_of, n_states=None, title="Filter visualisation"):
    """HTML of the records DeepQNetwork.visualize returns.  state_of(i) -> u8 [4, 84, 84]: state i of the visualised set (n_states of them)."""
    out = ["<!DOCTYPE html>", "<html><head><meta charset=\"utf-8\"><title>%s</title>" % html.escape(title),
           "<style>body{font-family:sans-serif} .fm{display:inline-block;margin:6px;text-align:center;font-size:12px}"
           " img{width:168px;height:168px;image-rendering:pixelated;margin:1px}</style></head><body>",
           "<h1>%s</h1>" % html.escape(title)]
    if n_states is not None:
        out.append("<p>%d states searched</p>" % n_states)
    for (name, kind), rec in zip(LAYERS, layers):
        out.append("<div class=\"layer\"><h2>%s (%s)</h2>" % (name, kind))
        for f in range(len(rec["value"])):
            n, p, v = int(rec["state"][f]), int(rec["pos"][f]), float(rec["value"][f])
            out.append("<div class=\"fm\"><div>Feature Map %d</div>"
                       "<img alt=\"projection\" src=\"%s\"><img alt=\"input\" src=\"%s\">"
                       "<div>state %d, position %d, activation %.4g</div></div>"
                       % (f, png_data_uri(encode_projection(rec["vis"][f])), png_data_uri(encode_state(state_of(n))), n, p, v))
        out.append("</div>")
    out.append("</body></html>")
    return "\n".join(out)


def visualize(net, mem_or_states, max_fm, filename, indexes=None):
    """The reference's visualize(model, data, max_fm, filename): mem_or_states is a ReplayMemory (with `indexes`: the ring indexes
    whose getState() is visualised, read on the device) or host states u8 [N, 4, 84, 84]."""
    if indexes is not None:
        mem = mem_or_states
        idx = np.asarray(indexes, dtype=np.int64).reshape(-1)
        layers, n = net.visualize(mem=mem, indexes=idx, max_fm=max_fm), idx.size

        def state_of(i):
            return np.asarray(mem.getState(int(idx[i])))
    else:
        states = np.asarray(mem_or_states, dtype=np.uint8)
        layers, n = net.visualize(states=states, max_fm=max_fm), len(states)

        def state_of(i):
            return states[i]
    page = summary_page(layers, state_of, n)
    with open(filename, "w") as f:
        f.write(page)
    logger.info("Wrote the filter visualisation of %d maps to %s" % (sum(len(r["value"]) for r in layers), filename))
    return layers
