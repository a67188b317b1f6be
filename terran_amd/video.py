"""Raw-video frame batches for the MI355X path.

Mirrors the reader contract of terran/io/video/reader.py:88-162,467-501: a `rawvideo` / `rgb24` byte stream
(what `ffmpeg ... -f rawvideo -pix_fmt rgb24 pipe:` writes) is cut into batches of `batch_size` frames of
`height x width x 3` bytes; a short final read yields a partial batch, a zero-length read ends the video; one
batch is prefetched by a daemon thread (DEFAULT_READER_BUFFER_SIZE = 1, io/video/__init__.py:6).

MI355X-first differences: the thread reads straight into page-locked host buffers (double-buffered) and
uploads on its OWN context/stream, so decode, H2D and the previous batch's kernels overlap; what the consumer
gets is a `lib.Frames` batch already resident in HBM (detection, recognition and pose all read it in place).
Building the ffmpeg command line (reader.py:421-465) stays Terran's job: pass its `proc.stdout` as `stream`.

The way out mirrors it: `JpegVideoWriter` encodes frames to JPEG on the GPU (terran_amd.image.encode_jpeg, byte for byte
Pillow's files) and writes them back to back -- a Motion-JPEG elementary stream, what `ffmpeg -f mjpeg -i pipe:` reads --
to `stream` (a file, or `proc.stdin` of an ffmpeg the caller started).  Only the compressed bytes leave the device.

Raw YUV: with `pix_fmt='yuv420p'` (or 'nv12', 'yuv444p') the reader takes what `ffmpeg ... -f rawvideo -pix_fmt yuv420p
pipe:` writes -- half the bytes of rgb24 through the pipe, the pinned buffers and the bus, and no swscale on the host --
and converts to RGB on the GPU (terran_amd.image.frames_from_yuv); `RawVideoWriter` converts resident frames back on the
GPU and writes raw frames for `ffmpeg -f rawvideo -pix_fmt yuv420p -s WxH -i pipe:`.  The conversion is the standards'
exact affine map, not swscale's arithmetic: see image.py.
"""
import threading
from queue import Full as QueueFull, Queue

import numpy as np

DEFAULT_READER_BUFFER_SIZE = 1
DEFAULT_WRITER_BUFFER_SIZE = 64                 # frames (terran/io/video/__init__.py)


class EndOfVideo(Exception):
    pass


class VideoClosed(Exception):
    pass


def read_batch(stream, out):
    """Fill `out` (batch, H, W, 3) uint8 from `stream`; returns the number of whole frames read
    (0 at end of stream).  Trailing bytes of an incomplete frame are dropped."""
    view = memoryview(out.reshape(-1))
    got = 0
    while got < len(view):
        n = stream.readinto(view[got:])
        if not n:
            break
        got += n
    return got // int(np.prod(out.shape[1:]))


RAW_PIX_FMTS = ('rgb24', 'yuv420p', 'nv12', 'yuv444p')


def raw_frame_bytes(pix_fmt, width, height):
    """The bytes of one raw frame (ffmpeg's rawvideo layout, no padding): 3 w h for 'rgb24', image.yuv_frame_bytes for
    the YUV formats.  ValueError for a format this module does not read, and for a YUV size outside 1 .. 65535 a side."""
    if pix_fmt not in RAW_PIX_FMTS:
        raise ValueError('pix_fmt must be one of %s, got %r' % (', '.join(repr(f) for f in RAW_PIX_FMTS), pix_fmt))
    if pix_fmt == 'rgb24':
        return 3 * width * height
    from . import image
    return image.yuv_frame_bytes(pix_fmt, (width, height))


class RawVideoReader:
    """Iterate device-resident frame batches from a raw rgb24 stream, or with `pix_fmt` 'yuv420p', 'nv12' or 'yuv444p'
    from a raw YUV stream that is converted to RGB on the GPU (`matrix`, `range`, `chroma`, `siting`: image.yuv_spec's).

        for frames in RawVideoReader(proc.stdout, 1920, 1080, batch_size=32):
            faces = face_detection(frames)          # lib.Frames go straight into the facades
    """

    def __init__(self, stream, width, height, batch_size=32, device=None, prefetch=DEFAULT_READER_BUFFER_SIZE,
                 upload=None, framerate=None, pix_fmt='rgb24', matrix='bt709', range='tv', chroma='bilinear', siting='left'):
        self.stream, self.width, self.height, self.batch_size = stream, int(width), int(height), int(batch_size)
        self.pix_fmt = pix_fmt
        self._frame_bytes = raw_frame_bytes(pix_fmt, self.width, self.height)       # a bad format fails here
        self._spec = None
        if pix_fmt != 'rgb24':
            from . import image
            self._spec = image.yuv_spec(pix_fmt, matrix, range, chroma, siting)
        self.framerate = framerate                 # frames per second of the source, as terran.io.video.Video exposes it
                                                   # (reader.py:229-236); `face_tracking(video=reader)` derives its ages from it
        self._queue = Queue(max(1, int(prefetch)))
        self._stop = threading.Event()
        self._closed = False
        self._error = None
        self._upload = upload                      # test hook: callable(ndarray) -> batch object
        self._device = device
        self._thread = threading.Thread(target=self._worker, daemon=True)
        self._thread.start()

    def _worker(self):
        ctx = bufs = None
        try:
            # rgb24: (batch, H, W, 3); a YUV format: (batch, frame bytes), the frames back to back
            shape = (self.batch_size, self.height, self.width, 3) if self._spec is None else (self.batch_size, self._frame_bytes)
            if self._upload is None:
                from . import affinity, runtime
                # this thread's memcpy into the pinned buffers, the buffers themselves (first touch) and the DMA out of them
                # stay on the NUMA node the GPU hangs off
                affinity.bind(runtime.device_index(self._device))
                ctx = runtime.new_context(self._device)            # own HIP stream: uploads overlap the consumer's kernels
                bufs = [ctx.pinned_array(shape) for _ in range(2)]
                arrays = [b[0] for b in bufs]
                if self._spec is None:
                    upload = ctx.upload
                else:
                    # H2D out of the pinned buffer into ta_frames_from_yuv's own staging block, then the kernel: nothing of this
                    # context that a consumer's call on the queued batches uses (its scratch and pinned blocks) is touched
                    def upload(raw):
                        return ctx.frames_from_yuv(raw, len(raw), self.height, self.width, self._spec)
            else:
                arrays = [np.empty(shape, np.uint8) for _ in range(2)]
                upload = self._upload
            i = 0
            while not self._stop.is_set():
                n = read_batch(self.stream, arrays[i])
                if n == 0:
                    break
                batch = upload(arrays[i][:n])                       # synchronous on this thread's stream
                while not self._stop.is_set():
                    try:
                        self._queue.put(batch, timeout=1.0)
                        break
                    except QueueFull:
                        continue
                i ^= 1
                if n < self.batch_size:
                    break
        except Exception as e:                                      # surfaced to the consumer
            self._error = e
        finally:
            while True:                                             # end-of-video sentinel; give up if the consumer closed
                try:
                    self._queue.put(None, timeout=0.2)
                    break
                except QueueFull:
                    if self._stop.is_set():
                        break
            if bufs:
                for _, ptr in bufs:
                    ctx.free_pinned(ptr)

    def __iter__(self):
        return self

    def __next__(self):
        if self._closed:
            raise VideoClosed()
        batch = self._queue.get()
        if batch is None:
            self._closed = True
            if self._error is not None:
                raise self._error
            raise StopIteration
        return batch

    def read(self):
        """Like `next()` but raises EndOfVideo at the end (the reference's explicit-read protocol)."""
        try:
            return next(self)
        except StopIteration:
            raise EndOfVideo()

    def close(self):
        self._stop.set()
        self._closed = True
        try:
            while self._queue.get_nowait() is not None:
                pass
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class JpegVideoWriter:
    """Write frames as a Motion-JPEG stream.

        with JpegVideoWriter(proc.stdin, quality=90) as writer:
            for frames in RawVideoReader(...):
                faces = face_detection(frames)
                vis.draw_faces(frames, faces)
                writer.write_frames(frames)            # encoded where they are; the bytes go to a writer thread

    Encoding runs on the calling thread's context (ordered after a draw on it); a daemon thread writes the files to
    `stream` through a queue of at most `buffer_size` frames.  A write error is raised by the next call; writing after
    `close()` raises VideoClosed.  `optimize`: Pillow's optimize=True, per-frame Huffman tables (a smaller stream).
    `encoder(images, quality, subsampling) -> list of bytes` replaces the GPU encoder (tests); with optimize=True it is
    called as `encoder(images, quality, subsampling, optimize=True)`."""

    def __init__(self, stream, quality=75, subsampling=-1, buffer_size=DEFAULT_WRITER_BUFFER_SIZE, device=None,
                 encoder=None, optimize=False):
        from . import image
        image.jpeg_options(quality, subsampling, optimize)  # bad options fail here, before any frame
        self.stream, self.quality, self.subsampling, self.optimize = stream, quality, subsampling, bool(optimize)
        self.frames_written = 0
        self._device = device
        self._encoder = encoder
        self._queue = Queue(max(1, int(buffer_size)))
        self._error = None
        self._closed = False
        self._thread = threading.Thread(target=self._worker, daemon=True)
        self._thread.start()

    def _worker(self):
        while True:
            data = self._queue.get()
            if data is None:
                break
            if self._error is not None:
                continue                                    # drain: the consumer sees the first error
            try:
                self.stream.write(data)
                self.frames_written += 1
            except Exception as e:                          # surfaced by the next call
                self._error = e
        if self._error is None:
            try:
                if hasattr(self.stream, 'flush'):
                    self.stream.flush()
            except Exception as e:
                self._error = e

    def _raise_pending(self):
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    def _encode(self, images):
        if self._encoder is not None:
            if self.optimize:
                return self._encoder(images, self.quality, self.subsampling, optimize=True)
            return self._encoder(images, self.quality, self.subsampling)
        from . import image
        return image.encode_jpeg(images, self.quality, self.subsampling, device=self._device, optimize=self.optimize)

    def write_frames(self, batch):
        """Encode every frame of `batch` (a lib.Frames batch, a list of them, or host uint8 (N, H, W, 3)) and queue the
        files."""
        if self._closed:
            raise VideoClosed('The video has already been closed.')
        self._raise_pending()
        for data in self._encode(batch):
            self._queue.put(data)

    def write_frame(self, frame_or_func, *args):
        """The reference's signature (terran/io/video/writer.py:122-156): a frame, or a function whose result
        `frame_or_func(*args)` is the frame (a host (H, W, 3) array or a resident batch)."""
        if self._closed:
            raise VideoClosed('The video has already been closed.')
        frame = frame_or_func(*args) if callable(frame_or_func) else frame_or_func
        self.write_frames(frame)

    def close(self):
        """Write what is queued, stop the thread; re-raises a pending write error."""
        if self._closed:
            raise VideoClosed('The video has already been closed.')
        self._closed = True
        self._queue.put(None)
        self._thread.join()
        self._raise_pending()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if not self._closed:
            self.close()


class RawVideoWriter:
    """Write frames as raw video, what `ffmpeg -f rawvideo -pix_fmt <pix_fmt> -s WxH -i pipe:` reads.

        with RawVideoWriter(proc.stdin, pix_fmt='yuv420p') as writer:
            for frames in RawVideoReader(..., pix_fmt='yuv420p'):
                vis.draw_faces(frames, face_detection(frames))
                writer.write_frames(frames)            # converted where they are; half of rgb24's bytes come back

    `pix_fmt` 'yuv420p', 'nv12' or 'yuv444p': the frames are converted on the GPU (terran_amd.image.frames_to_yuv; `matrix`
    and `range` are yuv_spec's) on the calling thread's context (runtime.get_context of `device`, or of the batch's device),
    never on the context of the reader thread that a reader's batch belongs to.  Every frame call is synchronous, so the
    conversion sees a draw that returned before it, whatever context the draw ran on.  'rgb24' writes the frames'
    bytes as they are, the contract of the reference's writer (terran/io/video/writer.py).  A daemon thread writes to
    `stream` through a queue of at most `buffer_size` frames; a write error is raised by the next call; writing after
    `close()` raises VideoClosed, a second `close()` does nothing.  `download(batch) -> uint8 (n, frame bytes)` replaces
    the conversion and the download (tests)."""

    def __init__(self, stream, pix_fmt='yuv420p', matrix='bt709', range='tv', buffer_size=DEFAULT_WRITER_BUFFER_SIZE, device=None,
                 download=None):
        raw_frame_bytes(pix_fmt, 1, 1)                      # a bad format fails here, before any frame
        self._spec_args = None
        if pix_fmt != 'rgb24':
            from . import image
            image.yuv_spec(pix_fmt, matrix, range)
            self._spec_args = (pix_fmt, matrix, range)
        self.stream, self.pix_fmt = stream, pix_fmt
        self.frames_written = 0
        self._device = device
        self._download = download
        self._queue = Queue(max(1, int(buffer_size)))
        self._error = None
        self._closed = False
        self._thread = threading.Thread(target=self._worker, daemon=True)
        self._thread.start()

    def _worker(self):
        while True:
            data = self._queue.get()
            if data is None:
                break
            if self._error is not None:
                continue                                    # drain: the consumer sees the first error
            try:
                self.stream.write(data)
                self.frames_written += 1
            except Exception as e:                          # surfaced by the next call
                self._error = e
        if self._error is None:
            try:
                if hasattr(self.stream, 'flush'):
                    self.stream.flush()
            except Exception as e:
                self._error = e

    def _raise_pending(self):
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    def _raw(self, batch):
        """The raw frames of `batch`, uint8 (n, frame bytes)."""
        if self._download is not None:
            raw = np.asarray(self._download(batch), np.uint8)
        elif self._spec_args is not None:
            from . import image
            raw = image.frames_to_yuv(batch, *self._spec_args, device=self._device)
        else:
            from . import lib
            if isinstance(batch, lib.Frames):
                raw = batch.download()
            elif isinstance(batch, (list, tuple)):
                if not batch or not all(isinstance(b, lib.Frames) for b in batch):
                    raise ValueError('write_frames: a list must hold lib.Frames batches')
                raw = np.concatenate([b.download().reshape(b.shape[0], -1) for b in batch])
            else:
                raw = np.ascontiguousarray(batch)
                if raw.dtype != np.uint8 or raw.ndim not in (3, 4) or raw.shape[-1] != 3 or 0 in raw.shape:
                    raise ValueError('write_frames: host images must be uint8 (H, W, 3) or (N, H, W, 3) RGB, got %s %s'
                                     % (raw.dtype, raw.shape))
                raw = raw[None] if raw.ndim == 3 else raw
        return np.ascontiguousarray(raw).reshape(len(raw), -1)

    def write_frames(self, batch):
        """Convert every frame of `batch` (a lib.Frames batch, a list of them, or host uint8 (N, H, W, 3)) and queue its
        bytes."""
        if self._closed:
            raise VideoClosed('The video has already been closed.')
        self._raise_pending()
        for frame in self._raw(batch):
            self._queue.put(memoryview(frame))

    def write_frame(self, frame_or_func, *args):
        """The reference's signature (terran/io/video/writer.py:122-156): a frame, or a function whose result
        `frame_or_func(*args)` is the frame (a host (H, W, 3) array or a resident batch)."""
        if self._closed:
            raise VideoClosed('The video has already been closed.')
        frame = frame_or_func(*args) if callable(frame_or_func) else frame_or_func
        self.write_frames(frame)

    def close(self):
        """Write what is queued, stop the thread; re-raises a pending write error.  Closing again does nothing."""
        if self._closed:
            return
        self._closed = True
        self._queue.put(None)
        self._thread.join()
        self._raise_pending()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
