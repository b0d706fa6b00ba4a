"""FrameBuffer::draw_line restated in pure Python from the reference's f_renderer/src/renderer.rs:540-588: the sequential
walk with its running remainder, and set_pixel's linear addressing (:497-503).  The line tests hold the library to this
file; it shares nothing with the package (neither the closed form of the kernels nor FrameBuffer.draw_line)."""

U32 = 0xFFFFFFFF


def iter_line_pixels(x1, y1, x2, y2):
    """The (x, y) arguments of every set_pixel call of draw_line(x1, y1, x2, y2, _), in call order (a generator)."""
    x1, x2 = (x1, x2) if x1 < x2 else (x2, x1)          # :541
    y1, y2 = (y1, y2) if y1 < y2 else (y2, y1)          # :542
    if x1 == x2 and y1 == y2:                           # :544-546
        yield x1, y1
    elif x1 == x2:                                      # :547-551
        for y in range(y1, y2):
            yield x1, y
    elif y1 == y2:                                      # :552-556
        for x in range(x1, x2):
            yield x, y1
    else:                                               # :557-586
        dx, dy = x2 - x1, y2 - y1
        rem = 0
        if dx > dy:
            y = y1
            for x in range(x1, x2):
                yield x, y
                rem += dy
                if rem >= dx:
                    y += 1
                    rem -= dx
                    yield x, y
            yield x2, y2
        else:
            x = x1
            for y in range(y1, y2):
                yield x, y
                rem += dx
                if rem >= dy:
                    x += 1
                    rem -= dy
                    yield x, y
            yield x2, y2


def line_pixels(x1, y1, x2, y2):
    return list(iter_line_pixels(x1, y1, x2, y2))


def line_indices(x1, y1, x2, y2, width):
    """Linear pixel indices y * width + x of the walk, in write order (set_pixel's offset / 4, :498)."""
    return [y * width + x for x, y in line_pixels(x1, y1, x2, y2)]


def panics(x1, y1, x2, y2, width, height):
    """Would the reference panic?  Its u32 offset arithmetic overflows (debug build), or an offset is past the buffer."""
    for x, y in iter_line_pixels(x1, y1, x2, y2):
        if y * width * 4 > U32 or x * 4 > U32 or y * width * 4 + x * 4 > U32:
            return True
        if y * width + x >= width * height:
            return True
    return False


def wireframe_segments(spi, width, height):
    """The list a host would build for frr_draw_wireframe from a setup list's spi [n, 3, 2] (emission-order vertices):
    segment 3t + e is edge e of triangle t, (v0,v1), (v1,v2), (v2,v0); an edge with an endpoint outside 0 <= x < width,
    0 <= y < height is skipped whole.  Returns (segments [(x1, y1, x2, y2)], skipped edges)."""
    segs, skipped = [], 0
    for tri in spi:
        for e in range(3):
            (xa, ya), (xb, yb) = tri[e], tri[(e + 1) % 3]
            if 0 <= xa < width and 0 <= xb < width and 0 <= ya < height and 0 <= yb < height:
                segs.append((xa, ya, xb, yb))
            else:
                skipped += 1
    return segs, skipped


def draw_line(image, x1, y1, x2, y2, color):
    """draw_line on a uint8 [H, W, 4] array, in place; IndexError where the reference panics (nothing is written then:
    callers compare whole lists, which the library refuses whole)."""
    h, w = image.shape[0], image.shape[1]
    if panics(x1, y1, x2, y2, w, h):
        raise IndexError("draw_line leaves the buffer")
    flat = image.reshape(-1, 4)
    for p in line_indices(x1, y1, x2, y2, w):
        flat[p] = color
    return image


def draw_lines(image, xyxy, rgba, row_filter=None):
    """Every segment of a list in order; row_filter(y) -> bool restricts the pixel rows written (a partitioned rank)."""
    h, w = image.shape[0], image.shape[1]
    flat = image.reshape(-1, 4)
    for (x1, y1, x2, y2), c in zip(xyxy, rgba):
        if panics(int(x1), int(y1), int(x2), int(y2), w, h):
            raise IndexError("draw_line leaves the buffer")
        for p in line_indices(int(x1), int(y1), int(x2), int(y2), w):
            if row_filter is None or row_filter(p // w):
                flat[p] = c
    return image
