"""Filter visualisation, host side: the command line of the reference's nvis.sh, the stdlib PNG encoder, the uint8 encoding of a
projection and the self-contained HTML page (no GPU needed)."""
import base64
import re
import struct
import zlib

import numpy as np

from simple_dqn_amd import main as M
from simple_dqn_amd import visualization as V


def _decode_png(data):
    """Minimal PNG reader for what png_bytes writes: -> (width, height, color type, pixel bytes without the filter bytes)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, color = ihdr[:4]
    assert depth == 8
    raw = zlib.decompress(idat)
    stride = w * (3 if color == 2 else 1)
    rows = [raw[y * (stride + 1):(y + 1) * (stride + 1)] for y in range(h)]
    assert all(r[0] == 0 for r in rows)
    return w, h, color, b"".join(r[1:] for r in rows)


def test_parser_accepts_nvis_command_line():
    # nvis.sh: main.py --play_games 1 --visualization_file results/$game.html --load_weights <snapshot>
    a = M.build_parser().parse_args(["breakout", "--play_games", "1", "--visualization_file", "results/breakout.html",
                                     "--load_weights", "snapshots/breakout_77.pkl"])
    assert a.visualization_file == "results/breakout.html" and a.visualization_filters == 4 and a.play_games == 1
    a = M.build_parser().parse_args(["--visualization_filters", "2"])
    assert a.visualization_filters == 2 and a.visualization_file is None


def test_png_round_trip():
    rng = np.random.RandomState(0)
    for img in (rng.randint(0, 256, (84, 84, 3)).astype(np.uint8), rng.randint(0, 256, (5, 7)).astype(np.uint8)):
        w, h, color, px = _decode_png(V.png_bytes(img))
        assert (w, h) == (img.shape[1], img.shape[0]) and color == (2 if img.ndim == 3 else 0)
        assert px == img.tobytes()


def test_encode_projection_truncates_and_scales():
    vis = np.zeros((4, 84, 84), np.float32)
    vis[0, 0, 0] = -1.0                      # channel 0: sets the minimum but is not shown
    vis[1, 2, 3] = 1.0                       # the maximum
    vis[2, 5, 5] = 0.0
    vis[3, 7, 7] = 0.5 - 1.0 / 255           # scales to 190.25 - 0.5: truncated
    img = V.encode_projection(vis)
    assert img.shape == (84, 84, 3) and img.dtype == np.uint8
    x = np.transpose(vis, (1, 2, 0)).astype(np.float32)
    want = ((x - x.min()) * (255.0 / (x.max() - x.min()))).astype(np.uint8)[:, :, 1:4]
    assert np.array_equal(img, want)
    assert img[2, 3, 0] == 255 and img[5, 5, 1] == 127 and img[0, 0, 0] == 127     # 0 -> 127.5 -> 127 (truncation, not rounding)
    assert img[7, 7, 2] == int((0.5 - 1.0 / 255 + 1.0) * 127.5)


def test_encode_projection_zero_range_and_channels():
    vis = np.full((4, 84, 84), 3.7, np.float32)
    assert np.array_equal(V.encode_projection(vis), np.full((84, 84, 3), 3, np.uint8))       # range 0: unscaled, truncated
    assert not V.encode_projection(np.zeros((4, 84, 84), np.float32)).any()
    st = np.arange(4 * 84 * 84, dtype=np.int64).reshape(4, 84, 84).astype(np.uint8)
    panel = V.encode_state(st)
    assert panel.shape == (84, 84, 3) and np.array_equal(panel[..., 0], st[1]) and np.array_equal(panel[..., 2], st[3])
    vis = np.zeros((4, 84, 84), np.float32)
    vis[0] = 9.0                                                  # only the dropped channel is non-zero
    img = V.encode_projection(vis)
    assert not img.any()


def _synthetic_layers(F, seed=1):
    rng = np.random.RandomState(seed)
    return [{"state": rng.randint(0, 10, f), "pos": rng.randint(0, 49, f), "value": rng.randn(f).astype(np.float32),
             "vis": rng.randn(f, 4, 84, 84).astype(np.float32)} for f in F]


def test_summary_page_structure():
    F = (3, 2, 4)
    states = np.random.RandomState(2).randint(0, 256, (10, 4, 84, 84)).astype(np.uint8)
    page = V.summary_page(_synthetic_layers(F), lambda i: states[i])
    for name in ("Layer 0000 (conv1)", "Layer 0002 (conv2)", "Layer 0004 (conv3)"):
        assert page.count(name) == 1
    blocks = page.split('<div class="layer">')[1:]
    assert len(blocks) == 3
    for blk, f in zip(blocks, F):
        assert [int(m) for m in re.findall(r"Feature Map (\d+)", blk)] == list(range(f))
    uris = re.findall(r'src="data:image/png;base64,([A-Za-z0-9+/=]+)"', page)
    assert len(uris) == 2 * sum(F)
    for u in uris:
        w, h, color, _ = _decode_png(base64.b64decode(u))
        assert (w, h, color) == (84, 84, 2)
    assert "http" not in page and "<script" not in page             # self-contained


def test_visualize_writes_page(tmp_path):
    class FakeNet:
        def visualize(self, states=None, mem=None, indexes=None, max_fm=4):
            assert mem is None and states.shape == (10, 4, 84, 84)
            return _synthetic_layers((min(32, max_fm), min(64, max_fm), min(64, max_fm)))
    states = np.zeros((10, 4, 84, 84), np.uint8)
    out = tmp_path / "v.html"
    layers = V.visualize(FakeNet(), states, 2, str(out))
    assert [len(r["value"]) for r in layers] == [2, 2, 2]
    page = out.read_text()
    assert page.count("data:image/png;base64,") == 12 and "<p>10 states searched</p>" in page
