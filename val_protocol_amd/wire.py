"""Host framing helpers (C implementation in csrc/val_wire.c).

``build_data_batch`` lays out a window of DATA frames the way the reference
sender emits them one by one (src/val_core.c:733-834); ``scan_frames`` walks a
received byte stream into descriptors for batch verify
(src/val_core.c:893-921).
"""
from __future__ import annotations

import ctypes

import numpy as np

from .crc import ValError, _check, lib

HEADER = 8
TRAILER = 4
VAL_PKT_DATA = 5
VAL_DATA_OFFSET_PRESENT = 1


def serialize_header(ptype: int, flags: int, content_len: int, type_data: int) -> bytes:
    out = (ctypes.c_uint8 * 8)()
    lib().val_serialize_frame_header(ptype, flags, content_len, type_data, out)
    return bytes(out)


def deserialize_header(hdr: bytes):
    buf = (ctypes.c_uint8 * 8).from_buffer_copy(hdr[:8])
    t, f = ctypes.c_uint8(), ctypes.c_uint8()
    cl, td = ctypes.c_uint16(), ctypes.c_uint32()
    lib().val_deserialize_frame_header(buf, ctypes.byref(t), ctypes.byref(f), ctypes.byref(cl), ctypes.byref(td))
    return t.value, f.value, cl.value, td.value


def build_data_batch(payload: np.ndarray, pay_off, pay_len, file_off, include_offset=None):
    """Returns (stream uint8, frame_off uint64, crc_len uint32); trailers zero."""
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    pay_len = np.ascontiguousarray(pay_len, dtype=np.uint32)
    file_off = np.ascontiguousarray(file_off, dtype=np.uint64)
    n = pay_len.size
    inc = None
    if include_offset is not None:
        inc = np.ascontiguousarray(include_offset, dtype=np.uint8)
    cap = int(pay_len.sum()) + n * (HEADER + 8 + TRAILER)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    frame_off = np.zeros(n, dtype=np.uint64)
    crc_len = np.zeros(n, dtype=np.uint32)
    used = ctypes.c_size_t(0)
    st = lib().val_frame_data_batch(payload.ctypes.data if payload.size else None, pay_off.ctypes.data,
                                    pay_len.ctypes.data, file_off.ctypes.data,
                                    inc.ctypes.data if inc is not None else None, n, out.ctypes.data, out.size,
                                    frame_off.ctypes.data, crc_len.ctypes.data, ctypes.byref(used))
    _check(st, "val_frame_data_batch")
    return out[: used.value], frame_off, crc_len


def put_trailers(stream: np.ndarray, frame_off, crc_len, crc) -> None:
    frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
    crc_len = np.ascontiguousarray(crc_len, dtype=np.uint32)
    crc = np.ascontiguousarray(crc, dtype=np.uint32)
    lib().val_frame_put_trailers(stream.ctypes.data, frame_off.ctypes.data, crc_len.ctypes.data, crc.ctypes.data,
                                 crc.size)


def data_layout(pay_len, include_offset=None):
    """Where build_data_batch puts each frame (val_frame_data_layout; host only):
    returns (frame_off uint64, crc_len uint32, total bytes)."""
    pay_len = np.ascontiguousarray(pay_len, dtype=np.uint32)
    n = pay_len.size
    inc = None
    if include_offset is not None:
        inc = np.ascontiguousarray(include_offset, dtype=np.uint8)
    frame_off = np.zeros(n, dtype=np.uint64)
    crc_len = np.zeros(n, dtype=np.uint32)
    total = ctypes.c_uint64(0)
    st = lib().val_frame_data_layout(pay_len.ctypes.data, inc.ctypes.data if inc is not None else None, n,
                                     frame_off.ctypes.data, crc_len.ctypes.data, ctypes.byref(total))
    _check(st, "val_frame_data_layout")
    return frame_off, crc_len, int(total.value)


def build_data_batch_dev(payload, pay_off, pay_len, file_off, include_offset=None, *, out, frame_off=None,
                         out_stride: int = 0, len_hint: int = 0, out_crc=None, out_hdr=None, nrejected=None,
                         stream=None):
    """Frame a window on the GPU, trailers included (val_frame_data_batch_dev):
    one launch on torch's current stream (or ``stream``), returns at once.

    All arguments are GPU tensors: ``payload`` and ``out`` uint8, ``pay_off``,
    ``file_off`` and ``frame_off`` int64 (uint64 bit patterns), ``pay_len``
    int32, ``include_offset`` uint8 (None: every frame explicit). Frames go to
    ``frame_off`` (data_layout gives the back-to-back stream) or, without it,
    to slots of ``out_stride`` bytes. Returns (crc_len, crc, nrejected): int32
    tensors of n, n and 1 entries; ``out_hdr`` (int32, n) receives header_crc.
    ``nrejected`` (int32[1], the caller's, already on the stream) is
    incremented instead of a fresh zeroed counter.
    """
    import torch

    from .crc import _dptr, _stream_ptr

    n = int(pay_len.numel())
    dev = out.device
    crc_len = torch.empty(n, dtype=torch.int32, device=dev)
    if out_crc is None:
        out_crc = torch.empty(n, dtype=torch.int32, device=dev)
    nrej = nrejected
    if nrej is None:
        nrej = torch.zeros(1, dtype=torch.int32, device=dev)
        if stream is not None:  # the counter's zero fill is ordered before the launch
            nrej.record_stream(stream)
            stream.wait_stream(torch.cuda.current_stream(dev))
    st = lib().val_frame_data_batch_dev(_dptr(payload), _dptr(pay_off), _dptr(pay_len), _dptr(file_off),
                                        _dptr(include_offset), n, _dptr(out), _dptr(frame_off), out_stride, len_hint,
                                        _dptr(crc_len), _dptr(out_crc), _dptr(out_hdr), _dptr(nrej),
                                        _stream_ptr(stream))
    _check(st, "val_frame_data_batch_dev")
    return crc_len, out_crc, nrej


NOT_ACCEPTED = (1 << 64) - 1  # VAL_FRAME_NOT_ACCEPTED (val_wire.h)


def frame_accept(file_off, pay_len, written: int, file_cap: int = (1 << 64) - 1, ok=None):
    """The receiver's ordering rule over a scanned batch (val_frame_accept; host
    only): ``file_off`` from data_offsets, ``pay_len`` from payload_lens, ``ok``
    the trailer verdicts (None: all good). Returns (dst_off uint64 with
    NOT_ACCEPTED for skipped frames, written, n_accepted, n_overflow)."""
    file_off = np.ascontiguousarray(file_off, dtype=np.uint64)
    pay_len = np.ascontiguousarray(pay_len, dtype=np.uint32)
    n = pay_len.size
    okp = None
    if ok is not None:
        ok = np.ascontiguousarray(ok, dtype=np.uint8)
        okp = ok.ctypes.data
    dst = np.zeros(n, dtype=np.uint64)
    w = ctypes.c_uint64(written)
    nacc, novf = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().val_frame_accept(file_off.ctypes.data, pay_len.ctypes.data, okp, n, file_cap, ctypes.byref(w),
                           dst.ctypes.data, ctypes.byref(nacc), ctypes.byref(novf))
    return dst, int(w.value), int(nacc.value), int(novf.value)


def unpack_work_bytes(n: int) -> int:
    """Workspace bytes unpack_data_batch_dev needs for n frames."""
    return int(lib().val_frame_unpack_work_bytes(n))


def unpack_data_batch_dev(base, *, file, written, off=None, length=None, stride: int = 0, flen: int = 0, n=None,
                          len_hint: int = 0, file_cap=None, file_state=None, out_ok=None, nbad=None, accept=None,
                          naccepted=None, noverflow=None, work=None, stream=None):
    """Verify a window of received frames and deliver the accepted payloads
    into a GPU-resident file (val_frame_unpack_batch_dev): a few launches on
    torch's current stream (or ``stream``), returns at once.

    All tensors live on the GPU. ``base`` uint8 and frames as in
    crc.verify_frames (``off`` int64 / ``length`` int32, or strided with
    ``stride``/``flen``/``n``). ``file`` uint8 (``file_cap``: its capacity,
    default its size); ``written`` int64[1] and ``file_state`` int32[1] (raw
    register, optional) are read and updated in place, so calls chain.
    ``out_ok`` / ``accept`` uint8[n] and the counters ``nbad``, ``naccepted``,
    ``noverflow`` (int32[1], incremented) are allocated (counters zeroed) when
    not given; ``work`` is the workspace (uint8, unpack_work_bytes(n)).
    Returns (ok, accept, nbad, naccepted, noverflow).
    """
    import torch

    from .crc import _dptr, _stream_ptr

    if n is None:
        n = int(off.numel()) if off is not None else 0
    dev = file.device
    if file_cap is None:
        file_cap = int(file.numel())
    fresh = []
    if out_ok is None:
        out_ok = torch.empty(n, dtype=torch.uint8, device=dev)
        fresh.append(out_ok)
    if accept is None:
        accept = torch.empty(n, dtype=torch.uint8, device=dev)
        fresh.append(accept)
    if work is None:
        work = torch.empty(max(unpack_work_bytes(n), 16), dtype=torch.uint8, device=dev)
        fresh.append(work)
    counters = []
    for c in (nbad, naccepted, noverflow):
        if c is None:
            c = torch.zeros(1, dtype=torch.int32, device=dev)
            fresh.append(c)
        counters.append(c)
    if stream is not None and fresh:  # allocations and zero fills are ordered before the launches
        for t in fresh:
            t.record_stream(stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
    st = lib().val_frame_unpack_batch_dev(_dptr(base), _dptr(off), _dptr(length), stride, flen, n, len_hint,
                                          _dptr(file), file_cap, _dptr(written), _dptr(file_state), _dptr(out_ok),
                                          _dptr(counters[0]), _dptr(accept), _dptr(counters[1]), _dptr(counters[2]),
                                          _dptr(work), int(work.numel()), _stream_ptr(stream))
    _check(st, "val_frame_unpack_batch_dev")
    return out_ok, accept, counters[0], counters[1], counters[2]


def unpack_data_files_dev(base, *, first, file_ptr, file_cap, written, off=None, length=None, stride: int = 0,
                          flen: int = 0, n=None, len_hint: int = 0, file_state=None, naccepted=None, noverflow=None,
                          file_nbad=None, out_ok=None, nbad=None, accept=None, work=None, stream=None):
    """Verify a window that holds frames of many files and deliver every
    file's accepted payloads (val_frame_unpack_files_dev): one verify, one
    parse, one order launch over the files and one scatter on torch's current
    stream (or ``stream``), returns at once. Per file the result is what
    unpack_data_batch_dev leaves for that file's frames alone.

    All tensors live on the GPU. ``base`` and the frames as in
    unpack_data_batch_dev; the descriptors are grouped by file: file s owns
    frames ``first[s]`` .. ``first[s + 1]`` (int32, S + 1 entries).
    ``file_ptr`` int64[S] holds the files' device addresses (``t.data_ptr()``
    of tensors the caller keeps alive), ``file_cap`` int64[S] their
    capacities; ``written`` int64[S] and ``file_state`` int32[S] (raw
    registers, optional) are read and updated in place, so calls chain.
    ``naccepted``, ``noverflow`` and ``file_nbad`` (int32[S], incremented),
    ``out_ok`` / ``accept`` uint8[n] and ``nbad`` (int32[1], incremented) are
    allocated (counters zeroed) when not given; ``work`` is the workspace
    (uint8, unpack_work_bytes(n)).
    Returns (ok, accept, nbad, naccepted, noverflow, file_nbad).
    """
    import torch

    from .crc import _dptr, _stream_ptr

    if n is None:
        n = int(off.numel()) if off is not None else 0
    n_files = int(written.numel())
    if int(first.numel()) != n_files + 1 or int(file_ptr.numel()) != n_files or int(file_cap.numel()) != n_files:
        raise ValueError("first needs one entry more than written; file_ptr and file_cap as many")
    dev = written.device
    fresh = []
    if out_ok is None:
        out_ok = torch.empty(n, dtype=torch.uint8, device=dev)
        fresh.append(out_ok)
    if accept is None:
        accept = torch.empty(n, dtype=torch.uint8, device=dev)
        fresh.append(accept)
    if work is None:
        work = torch.empty(max(unpack_work_bytes(n), 16), dtype=torch.uint8, device=dev)
        fresh.append(work)
    counters = []
    for c, size in ((nbad, 1), (naccepted, n_files), (noverflow, n_files), (file_nbad, n_files)):
        if c is None:
            c = torch.zeros(size, dtype=torch.int32, device=dev)
            fresh.append(c)
        counters.append(c)
    if stream is not None and fresh:  # allocations and zero fills are ordered before the launches
        for t in fresh:
            t.record_stream(stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
    st = lib().val_frame_unpack_files_dev(_dptr(base), _dptr(off), _dptr(length), stride, flen, n, len_hint, n_files,
                                          _dptr(first), _dptr(file_ptr), _dptr(file_cap), _dptr(written),
                                          _dptr(file_state), _dptr(counters[1]), _dptr(counters[2]),
                                          _dptr(counters[3]), _dptr(out_ok), _dptr(counters[0]), _dptr(accept),
                                          _dptr(work), int(work.numel()), _stream_ptr(stream))
    _check(st, "val_frame_unpack_files_dev")
    return out_ok, accept, counters[0], counters[1], counters[2], counters[3]


def scan_frames(stream: np.ndarray, mtu: int, max_frames: int = 1 << 30):
    """Returns (status, frame_off, crc_len, consumed)."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    cap = min(max_frames, stream.size // (HEADER + TRAILER) + 1)
    frame_off = np.zeros(cap, dtype=np.uint64)
    crc_len = np.zeros(cap, dtype=np.uint32)
    nf = ctypes.c_uint32(0)
    used = ctypes.c_size_t(0)
    st = lib().val_frame_scan(stream.ctypes.data, stream.size, mtu, cap, frame_off.ctypes.data, crc_len.ctypes.data,
                              ctypes.byref(nf), ctypes.byref(used))
    return st, frame_off[: nf.value], crc_len[: nf.value], used.value


def scan_work_bytes(n_streams: int, max_frames: int) -> int:
    """Workspace bytes scan_streams_dev needs."""
    return int(lib().val_frame_scan_work_bytes(n_streams, max_frames))


def scan_streams_dev(base, stream_off, stream_len, mtu: int, max_frames: int, *, stream=None):
    """scan_frames for S byte streams that lie on the GPU
    (val_frame_scan_streams_dev): three launches on torch's current stream (or
    ``stream``), returns at once.

    All tensors live on the GPU. Stream s is
    ``base[stream_off[s] : stream_off[s] + stream_len[s]]`` (``base`` uint8,
    ``stream_off`` / ``stream_len`` int64[S], uint64 bit patterns); at most
    ``max_frames`` frames are taken from each. Returns (frame_off, crc_len,
    first, nframes, consumed, status): ``frame_off`` int64 and ``crc_len``
    int32 of S * max_frames entries, the streams' descriptors one after the
    other with absolute offsets in ``base`` and (0, 0) behind the total;
    ``first`` int32[S + 1], stream s owning entries ``first[s]`` ..
    ``first[s + 1]``; ``nframes`` int32[S], ``consumed`` int64[S] (relative to
    the stream start) and ``status`` int32[S] (VAL_OK or VAL_ERR_PROTOCOL) as
    scan_frames reports them per stream. frame_off, crc_len and first feed
    unpack_data_files_dev as ``off``, ``length`` and ``first``; with
    ``n = S * max_frames`` nothing has to be read back in between (then read
    ``file_nbad``, not ``nbad``, and keep ``base`` at 4 bytes or more).
    """
    import torch

    from .crc import _dptr, _stream_ptr

    S = int(stream_off.numel())
    if int(stream_len.numel()) != S:
        raise ValueError("stream_off and stream_len need one entry per stream")
    slots = S * int(max_frames)
    dev = base.device
    frame_off = torch.empty(slots, dtype=torch.int64, device=dev)
    crc_len = torch.empty(slots, dtype=torch.int32, device=dev)
    first = torch.empty(S + 1, dtype=torch.int32, device=dev)
    nframes = torch.empty(S, dtype=torch.int32, device=dev)
    consumed = torch.empty(S, dtype=torch.int64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    work = torch.empty(max(scan_work_bytes(S, max_frames), 16), dtype=torch.uint8, device=dev)
    if stream is not None:  # the allocations are ordered before the launches
        for t in (frame_off, crc_len, first, nframes, consumed, status, work):
            t.record_stream(stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
    st = lib().val_frame_scan_streams_dev(_dptr(base), _dptr(stream_off), _dptr(stream_len), S, mtu, max_frames,
                                          _dptr(frame_off), _dptr(crc_len), _dptr(first), _dptr(nframes),
                                          _dptr(consumed), _dptr(status), _dptr(work), int(work.numel()),
                                          _stream_ptr(stream))
    _check(st, "val_frame_scan_streams_dev")
    return frame_off, crc_len, first, nframes, consumed, status


def fill_window(next: int, last_acked: int, file_size: int, mtu: int, budget: int, out_cap: int = (1 << 64) - 1):
    """The sender's window-fill rule (val_frame_fill_window; host only): the
    DATA frames a sender at file offset ``next`` puts into a window of at most
    ``budget`` frames and ``out_cap`` wire bytes; the first one carries its
    offset iff ``next == last_acked``. Returns (file_off uint64, pay_len
    uint32, include_offset uint8, frame_off uint64 relative to the stream
    start, crc_len uint32, used bytes, new next): the inputs of
    build_data_batch / build_data_batch_dev and their placement. Raises
    ValError for an mtu outside 21..65547."""
    file_off = np.zeros(budget, dtype=np.uint64)
    pay_len = np.zeros(budget, dtype=np.uint32)
    inc = np.zeros(budget, dtype=np.uint8)
    frame_off = np.zeros(budget, dtype=np.uint64)
    crc_len = np.zeros(budget, dtype=np.uint32)
    nf = ctypes.c_uint32(0)
    used, nxt = ctypes.c_uint64(0), ctypes.c_uint64(0)
    st = lib().val_frame_fill_window(next, last_acked, file_size, mtu, budget, out_cap, file_off.ctypes.data,
                                     pay_len.ctypes.data, inc.ctypes.data, frame_off.ctypes.data, crc_len.ctypes.data,
                                     ctypes.byref(nf), ctypes.byref(used), ctypes.byref(nxt))
    _check(st, "val_frame_fill_window")
    n = nf.value
    return file_off[:n], pay_len[:n], inc[:n], frame_off[:n], crc_len[:n], int(used.value), int(nxt.value)


def fill_work_bytes(n_files: int, max_frames: int) -> int:
    """Workspace bytes fill_files_dev needs."""
    return int(lib().val_frame_fill_work_bytes(n_files, max_frames))


def fill_files_dev(payload, file_pos, file_size, next, last_acked, mtu: int, max_frames: int, *, out, stream_off,
                   stream_cap, budget=None, out_hdr=None, work=None, stream=None):
    """fill_window plus build_data_batch_dev for S transfers whose files lie on
    the GPU (val_frame_fill_files_dev): four launches on torch's current
    stream (or ``stream``), returns at once.

    All tensors live on the GPU. File s is ``file_size[s]`` bytes at
    ``payload.data_ptr() + file_pos[s]`` (``payload`` uint8; ``file_pos``,
    ``file_size``, ``next``, ``last_acked`` int64[S], uint64 bit patterns;
    ``budget`` int32[S], None: ``max_frames`` each). The frames of transfer s
    go back to back to ``out[stream_off[s]:]``, at most ``stream_cap[s]``
    bytes (int64[S]); ``next`` is updated in place, so calls chain. Returns
    (frame_off, crc_len, crc, first, nframes, stream_len): ``frame_off`` int64
    (absolute in ``out``), ``crc_len`` and ``crc`` int32 of S * max_frames
    entries, the transfers' frames one after the other and zeros behind the
    total; ``first`` int32[S + 1]; ``nframes`` int32[S] and ``stream_len``
    int64[S]. ``out_hdr`` (int32, S * max_frames) receives header_crc.
    ``out``, frame_off, crc_len and first feed unpack_data_files_dev and
    crc.verify_frames; stream_off and stream_len feed scan_streams_dev.
    """
    import torch

    from .crc import _dptr, _stream_ptr

    S = int(next.numel())
    for t in (file_pos, file_size, last_acked, stream_off, stream_cap):
        if int(t.numel()) != S:
            raise ValueError("file_pos, file_size, next, last_acked, stream_off and stream_cap need one entry per transfer")
    if budget is not None and int(budget.numel()) != S:
        raise ValueError("budget needs one entry per transfer")
    slots = S * int(max_frames)
    dev = out.device
    frame_off = torch.empty(slots, dtype=torch.int64, device=dev)
    crc_len = torch.empty(slots, dtype=torch.int32, device=dev)
    crc = torch.empty(slots, dtype=torch.int32, device=dev)
    first = torch.empty(S + 1, dtype=torch.int32, device=dev)
    nframes = torch.empty(S, dtype=torch.int32, device=dev)
    stream_len = torch.empty(S, dtype=torch.int64, device=dev)
    fresh = [frame_off, crc_len, crc, first, nframes, stream_len]
    if work is None:
        work = torch.empty(max(fill_work_bytes(S, max_frames), 16), dtype=torch.uint8, device=dev)
        fresh.append(work)
    if stream is not None:  # the allocations are ordered before the launches
        for t in fresh:
            t.record_stream(stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
    st = lib().val_frame_fill_files_dev(_dptr(payload), _dptr(file_pos), _dptr(file_size), _dptr(next),
                                        _dptr(last_acked), _dptr(budget), S, mtu, max_frames, _dptr(out),
                                        _dptr(stream_off), _dptr(stream_cap), _dptr(stream_len), _dptr(nframes),
                                        _dptr(first), _dptr(frame_off), _dptr(crc_len), _dptr(crc), _dptr(out_hdr),
                                        _dptr(work), int(work.numel()), _stream_ptr(stream))
    _check(st, "val_frame_fill_files_dev")
    return frame_off, crc_len, crc, first, nframes, stream_len


def resume_tail_window(existing: int, incoming: int, tail_cap_bytes: int = 0, min_verify_bytes: int = 0,
                       mismatch_skip: bool = False):
    """The receiver's resume proposal under VAL_RESUME_TAIL
    (val_resume_tail_window; host only). Returns (action, resume_offset,
    verify_len): for VAL_RESUME_VERIFY_FIRST (2) the window to hash is
    [existing - verify_len, existing); for every other action both are 0."""
    off, vlen = ctypes.c_uint64(0), ctypes.c_uint64(0)
    action = lib().val_resume_tail_window(existing, incoming, tail_cap_bytes, min_verify_bytes, int(mismatch_skip),
                                          ctypes.byref(off), ctypes.byref(vlen))
    return int(action), int(off.value), int(vlen.value)


def resume_request_window(resume_offset: int, verify_len: int):
    """The sender's clamp of a VERIFY_FIRST answer (val_resume_request_window;
    host only). Returns (send, start, vlen32): send is False when the window is
    empty (no VERIFY goes out; the transfer starts at resume_offset)."""
    start, v32 = ctypes.c_uint64(0), ctypes.c_uint32(0)
    send = lib().val_resume_request_window(resume_offset, verify_len, ctypes.byref(start), ctypes.byref(v32))
    return bool(send), int(start.value), int(v32.value)


def resume_verdict(window_ok: bool, local_crc: int, sender_crc: int, mismatch_skip: bool, rec_resume_off: int,
                   file_size: int):
    """The receiver's VERIFY result and the offset it resumes at
    (val_resume_verdict; host only). Returns (status, resume_offset)."""
    off = ctypes.c_uint64(0)
    st = lib().val_resume_verdict(int(bool(window_ok)), local_crc & 0xFFFFFFFF, sender_crc & 0xFFFFFFFF,
                                  int(mismatch_skip), rec_resume_off, file_size, ctypes.byref(off))
    return int(st), int(off.value)


def file_windows_work_bytes(n_files: int) -> int:
    """Workspace bytes file_windows_dev and the resume calls need."""
    return int(lib().val_file_windows_work_bytes(n_files))


def _windows_call(fresh, work, stream, dev, n_files):
    """The workspace and the stream ordering the file-window wrappers share."""
    import torch

    if work is None:
        work = torch.empty(max(file_windows_work_bytes(n_files), 16), dtype=torch.uint8, device=dev)
        fresh = fresh + [work]
    if stream is not None:  # the allocations are ordered before the launches
        for t in fresh:
            t.record_stream(stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
    return work


def _per_file(n, **tensors):
    for name, t in tensors.items():
        if t is not None and int(t.numel()) != n:
            raise ValueError(f"{name} needs one entry per file")


def file_windows_dev(file_ptr, file_size, win_off, win_len, max_len: int, *, want_status: bool = True, work=None,
                     stream=None):
    """CRC-32 of one window per GPU-resident file (val_crc32_file_windows_dev):
    three launches on torch's current stream (or ``stream``), returns at once.

    ``file_ptr`` (device addresses), ``file_size``, ``win_off`` and ``win_len``
    are int64[S] tensors on the GPU holding uint64 bit patterns. Returns
    (crc int32[S], status int32[S] or None): the finalized CRC of
    ``[win_off, win_off + win_len)`` of each file; a window outside its file
    or longer than ``max_len`` gets status VAL_ERR_INVALID_ARG and crc 0, and
    none of its bytes is read."""
    import torch

    from .crc import _dptr, _stream_ptr

    S = int(file_ptr.numel())
    _per_file(S, file_size=file_size, win_off=win_off, win_len=win_len)
    dev = file_ptr.device
    crc = torch.empty(S, dtype=torch.int32, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev) if want_status else None
    work = _windows_call([crc] + ([status] if want_status else []), work, stream, dev, S)
    st = lib().val_crc32_file_windows_dev(_dptr(file_ptr), _dptr(file_size), _dptr(win_off), _dptr(win_len), S, max_len,
                                          _dptr(crc), _dptr(status), _dptr(work), int(work.numel()),
                                          _stream_ptr(stream))
    _check(st, "val_crc32_file_windows_dev")
    return crc, status


def resume_tail_files_dev(file_ptr, existing, incoming, *, tail_cap_bytes: int = 0, min_verify_bytes: int = 0,
                          mismatch_skip: bool = False, work=None, stream=None):
    """The receiver's resume proposal for S GPU-resident files
    (val_resume_tail_files_dev): resume_tail_window per file, and the tail
    window's CRC for VERIFY_FIRST files. ``existing`` (int64[S]) can be the
    ``written`` of unpack_data_files_dev on the same stream. Returns (action
    int32[S], resume_off int64[S], verify_len int64[S], verify_crc int32[S])."""
    import torch

    from .crc import _dptr, _stream_ptr

    S = int(file_ptr.numel())
    _per_file(S, existing=existing, incoming=incoming)
    dev = file_ptr.device
    action = torch.empty(S, dtype=torch.int32, device=dev)
    resume_off = torch.empty(S, dtype=torch.int64, device=dev)
    verify_len = torch.empty(S, dtype=torch.int64, device=dev)
    verify_crc = torch.empty(S, dtype=torch.int32, device=dev)
    work = _windows_call([action, resume_off, verify_len, verify_crc], work, stream, dev, S)
    st = lib().val_resume_tail_files_dev(_dptr(file_ptr), _dptr(existing), _dptr(incoming), S, tail_cap_bytes,
                                         min_verify_bytes, int(mismatch_skip), _dptr(action), _dptr(resume_off),
                                         _dptr(verify_len), _dptr(verify_crc), _dptr(work), int(work.numel()),
                                         _stream_ptr(stream))
    _check(st, "val_resume_tail_files_dev")
    return action, resume_off, verify_len, verify_crc


def resume_request_files_dev(file_ptr, file_size, action, resume_off, verify_len, max_len: int, *,
                             want_status: bool = True, work=None, stream=None):
    """The sender's answer for S GPU-resident files
    (val_resume_request_files_dev): resume_request_window per VERIFY_FIRST
    file and the CRC of that window of the sender's file. Returns (req_off
    int64[S], req_len int32[S], req_crc int32[S], status int32[S] or None);
    files with another action or an empty window get (resume_off, 0, 0,
    VAL_OK)."""
    import torch

    from .crc import _dptr, _stream_ptr

    S = int(file_ptr.numel())
    _per_file(S, file_size=file_size, action=action, resume_off=resume_off, verify_len=verify_len)
    dev = file_ptr.device
    req_off = torch.empty(S, dtype=torch.int64, device=dev)
    req_len = torch.empty(S, dtype=torch.int32, device=dev)
    req_crc = torch.empty(S, dtype=torch.int32, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev) if want_status else None
    work = _windows_call([req_off, req_len, req_crc] + ([status] if want_status else []), work, stream, dev, S)
    st = lib().val_resume_request_files_dev(_dptr(file_ptr), _dptr(file_size), _dptr(action), _dptr(resume_off),
                                            _dptr(verify_len), S, max_len, _dptr(req_off), _dptr(req_len),
                                            _dptr(req_crc), _dptr(status), _dptr(work), int(work.numel()),
                                            _stream_ptr(stream))
    _check(st, "val_resume_request_files_dev")
    return req_off, req_len, req_crc, status


def resume_check_files_dev(file_ptr, existing, incoming, req_off, req_len, req_crc, rec_resume_off, max_len: int, *,
                           result, written, action=None, local_crc=None, mismatch_skip: bool = False, work=None,
                           stream=None):
    """The receiver's check of the VERIFY requests of S GPU-resident files
    (val_resume_check_files_dev): the CRC of the requested window of the local
    file and resume_verdict. For VERIFY_FIRST files (``action`` None: all)
    ``result`` (int32[S]), ``written`` (int64[S]: the offset the transfer
    resumes at) and ``local_crc`` (int32[S], optional) are written in place;
    the entries of every other file keep their values. ``written`` then feeds
    unpack_data_files_dev, and ``next`` / ``last_acked`` of fill_files_dev on
    the peer."""
    from .crc import _dptr, _stream_ptr

    S = int(file_ptr.numel())
    _per_file(S, existing=existing, incoming=incoming, req_off=req_off, req_len=req_len, req_crc=req_crc,
              rec_resume_off=rec_resume_off, result=result, written=written, action=action, local_crc=local_crc)
    work = _windows_call([], work, stream, file_ptr.device, S)
    st = lib().val_resume_check_files_dev(_dptr(file_ptr), _dptr(existing), _dptr(incoming), _dptr(action),
                                          _dptr(req_off), _dptr(req_len), _dptr(req_crc), _dptr(rec_resume_off), S,
                                          max_len, int(mismatch_skip), _dptr(local_crc), _dptr(result), _dptr(written),
                                          _dptr(work), int(work.numel()), _stream_ptr(stream))
    _check(st, "val_resume_check_files_dev")
    return result, written, local_crc


PKT_DATA_ACK, PKT_DATA_NAK = 6, 13
NAK_REASON_GAP = 1


def put_response(kind: int, offset: int, reason: int = NAK_REASON_GAP) -> bytes:
    """One DATA_ACK (6) or DATA_NAK (13) frame for ``offset`` with its trailer
    (val_frame_put_response; host only): 12 or 16 bytes for an ACK, 24 for a
    NAK; b"" for another kind."""
    out = (ctypes.c_uint8 * 24)()
    used = lib().val_frame_put_response(kind, offset, reason, out)
    return bytes(out[:used])


def ack_offsets(stream: np.ndarray, frame_off, crc_len):
    """Kind (6, 13 or 0) and acknowledged offset of each scanned frame
    (val_frame_ack_offsets). Returns (kind uint8, ack_off uint64)."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
    crc_len = np.ascontiguousarray(crc_len, dtype=np.uint32)
    kind = np.zeros(crc_len.size, dtype=np.uint8)
    off = np.zeros(crc_len.size, dtype=np.uint64)
    lib().val_frame_ack_offsets(stream.ctypes.data, frame_off.ctypes.data, crc_len.ctypes.data, crc_len.size,
                                kind.ctypes.data, off.ctypes.data)
    return kind, off


def respond_window(file_off, pay_len, written: int, total: int, ack_stride: int = 1, since: int = 0,
                   file_cap: int = (1 << 64) - 1, ok=None):
    """The receiver's answer to one file's window (val_frame_respond_window;
    host only): inputs as frame_accept, plus the incoming file's size
    ``total``, the ACK stride (0: one ACK per window) and ``since``, the frames
    accepted since the last stride ACK. Returns (resp_frame uint32, resp_kind
    uint8, resp_off uint64, written, since): the responses in frame order."""
    file_off = np.ascontiguousarray(file_off, dtype=np.uint64)
    pay_len = np.ascontiguousarray(pay_len, dtype=np.uint32)
    n = pay_len.size
    okp = None
    if ok is not None:
        ok = np.ascontiguousarray(ok, dtype=np.uint8)
        okp = ok.ctypes.data
    frame = np.zeros(2 * n, dtype=np.uint32)
    kind = np.zeros(2 * n, dtype=np.uint8)
    off = np.zeros(2 * n, dtype=np.uint64)
    w, s, nr = ctypes.c_uint64(written), ctypes.c_uint32(since), ctypes.c_uint32(0)
    lib().val_frame_respond_window(file_off.ctypes.data, pay_len.ctypes.data, okp, n, file_cap, total, ack_stride,
                                   ctypes.byref(w), ctypes.byref(s), frame.ctypes.data, kind.ctypes.data,
                                   off.ctypes.data, ctypes.byref(nr))
    r = nr.value
    return frame[:r], kind[:r], off[:r], int(w.value), int(s.value)


def apply_acks(kind, ack_off, file_size: int, last_acked: int, next: int, ok=None):
    """The sender's handling of one transfer's response window
    (val_frame_apply_acks; host only): ``kind`` / ``ack_off`` from ack_offsets,
    ``ok`` the trailer verdicts (None: all good). Returns (last_acked, next,
    n_retrans, n_crc)."""
    kind = np.ascontiguousarray(kind, dtype=np.uint8)
    ack_off = np.ascontiguousarray(ack_off, dtype=np.uint64)
    okp = None
    if ok is not None:
        ok = np.ascontiguousarray(ok, dtype=np.uint8)
        okp = ok.ctypes.data
    la, nx = ctypes.c_uint64(last_acked), ctypes.c_uint64(next)
    nr, nc = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().val_frame_apply_acks(kind.ctypes.data, ack_off.ctypes.data, okp, kind.size, file_size, ctypes.byref(la),
                               ctypes.byref(nx), ctypes.byref(nr), ctypes.byref(nc))
    return int(la.value), int(nx.value), int(nr.value), int(nc.value)


def respond_bytes_max(frames: int) -> int:
    """Bound on the response bytes of a file that owns ``frames`` frames."""
    return int(lib().val_frame_respond_bytes_max(frames))


def respond_work_bytes(n: int) -> int:
    """Workspace bytes respond_files_dev needs for n frames."""
    return int(lib().val_frame_respond_work_bytes(n))


def apply_acks_work_bytes(n: int) -> int:
    """Workspace bytes apply_acks_files_dev needs for n frames."""
    return int(lib().val_frame_apply_acks_work_bytes(n))


def respond_files_dev(base, *, first, ok, accept, written, total, out, resp_off, resp_cap, ack_stride: int = 1,
                      since=None, off=None, length=None, stride: int = 0, flen: int = 0, n=None, ndropped=None,
                      work=None, stream=None):
    """Answer a delivered window with DATA_ACK / DATA_NAK frames on the GPU
    (val_frame_respond_files_dev): call it right after unpack_data_files_dev
    on the same stream, with the same frames and ``first`` and that call's
    ``ok``, ``accept`` and ``written``. Three launches, returns at once.

    All tensors live on the GPU. ``total`` int64[S] holds the incoming files'
    sizes; ``since`` int32[S] (needed unless ``ack_stride`` is 0) is updated in
    place. The responses of file s go back to back to ``out[resp_off[s]:]``,
    at most ``resp_cap[s]`` bytes (int64[S]; respond_bytes_max bounds them).
    Returns (resp_len int64[S], nresp int32[S], ndropped int32[S]); ``out``,
    resp_off and resp_len feed scan_streams_dev."""
    import torch

    from .crc import _dptr, _stream_ptr

    if n is None:
        n = int(off.numel()) if off is not None else 0
    S = int(written.numel())
    _per_file(S, total=total, resp_off=resp_off, resp_cap=resp_cap, since=since, ndropped=ndropped)
    if int(first.numel()) != S + 1:
        raise ValueError("first needs one entry more than written")
    dev = written.device
    resp_len = torch.zeros(S, dtype=torch.int64, device=dev)
    nresp = torch.zeros(S, dtype=torch.int32, device=dev)
    fresh = [resp_len, nresp]
    if ndropped is None:
        ndropped = torch.zeros(S, dtype=torch.int32, device=dev)
        fresh.append(ndropped)
    if work is None:
        work = torch.empty(max(respond_work_bytes(n), 16), dtype=torch.uint8, device=dev)
        fresh.append(work)
    if stream is not None:  # allocations and zero fills are ordered before the launches
        for t in fresh:
            t.record_stream(stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
    st = lib().val_frame_respond_files_dev(_dptr(base), _dptr(off), _dptr(length), stride, flen, n, S, _dptr(first),
                                           _dptr(ok), _dptr(accept), _dptr(written), _dptr(total), ack_stride,
                                           _dptr(since), _dptr(out), _dptr(resp_off), _dptr(resp_cap),
                                           _dptr(resp_len), _dptr(nresp), _dptr(ndropped), _dptr(work),
                                           int(work.numel()), _stream_ptr(stream))
    _check(st, "val_frame_respond_files_dev")
    return resp_len, nresp, ndropped


def apply_acks_files_dev(base, *, first, file_size, last_acked, next, off=None, length=None, stride: int = 0,
                         flen: int = 0, n=None, len_hint: int = 0, nretrans=None, file_nbad=None, out_ok=None,
                         nbad=None, work=None, stream=None):
    """Apply a window of received DATA_ACK / DATA_NAK frames to the send state
    of S transfers on the GPU (val_frame_apply_acks_files_dev): the verify
    launches and one apply launch, returns at once.

    All tensors live on the GPU; the frames and ``first`` as scan_streams_dev
    returns them. ``last_acked`` and ``next`` (int64[S]) are updated in place
    and feed fill_files_dev. ``nretrans`` / ``file_nbad`` (int32[S],
    incremented) are allocated zeroed when not given. Returns (nretrans,
    file_nbad)."""
    import torch

    from .crc import _dptr, _stream_ptr

    if n is None:
        n = int(off.numel()) if off is not None else 0
    S = int(last_acked.numel())
    _per_file(S, file_size=file_size, next=next, nretrans=nretrans, file_nbad=file_nbad)
    if int(first.numel()) != S + 1:
        raise ValueError("first needs one entry more than last_acked")
    dev = last_acked.device
    fresh = []
    if nretrans is None:
        nretrans = torch.zeros(S, dtype=torch.int32, device=dev)
        fresh.append(nretrans)
    if file_nbad is None:
        file_nbad = torch.zeros(S, dtype=torch.int32, device=dev)
        fresh.append(file_nbad)
    if work is None:
        work = torch.empty(max(apply_acks_work_bytes(n), 16), dtype=torch.uint8, device=dev)
        fresh.append(work)
    if stream is not None and fresh:  # allocations and zero fills are ordered before the launches
        for t in fresh:
            t.record_stream(stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
    st = lib().val_frame_apply_acks_files_dev(_dptr(base), _dptr(off), _dptr(length), stride, flen, n, len_hint, S,
                                              _dptr(first), _dptr(file_size), _dptr(last_acked), _dptr(next),
                                              _dptr(nretrans), _dptr(file_nbad), _dptr(out_ok), _dptr(nbad),
                                              _dptr(work), int(work.numel()), _stream_ptr(stream))
    _check(st, "val_frame_apply_acks_files_dev")
    return nretrans, file_nbad


def payload_lens(stream: np.ndarray, frame_off, crc_len) -> np.ndarray:
    """Payload bytes of each frame (val_frame_payload_lens)."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
    crc_len = np.ascontiguousarray(crc_len, dtype=np.uint32)
    out = np.zeros(crc_len.size, dtype=np.uint32)
    lib().val_frame_payload_lens(stream.ctypes.data, frame_off.ctypes.data, crc_len.ctypes.data, crc_len.size,
                                 out.ctypes.data)
    return out


# val_frame_data_offsets sentinels (val_wire.h)
OFFSET_IMPLIED = (1 << 64) - 1
OFFSET_NOT_DATA = (1 << 64) - 2


def data_offsets(stream: np.ndarray, frame_off, crc_len) -> np.ndarray:
    """File offset of each frame as the receiver reads it (val_frame_data_offsets):
    explicit offset, OFFSET_IMPLIED or OFFSET_NOT_DATA."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
    crc_len = np.ascontiguousarray(crc_len, dtype=np.uint32)
    out = np.zeros(crc_len.size, dtype=np.uint64)
    lib().val_frame_data_offsets(stream.ctypes.data, frame_off.ctypes.data, crc_len.ctypes.data, crc_len.size,
                                 out.ctypes.data)
    return out


__all__ = ["serialize_header", "deserialize_header", "build_data_batch", "build_data_batch_dev", "data_layout",
           "unpack_data_batch_dev", "unpack_data_files_dev", "unpack_work_bytes", "frame_accept", "NOT_ACCEPTED", "put_trailers", "scan_frames", "scan_streams_dev", "scan_work_bytes", "payload_lens",
           "fill_window", "fill_files_dev", "fill_work_bytes",
           "resume_tail_window", "resume_request_window", "resume_verdict", "file_windows_dev",
           "resume_tail_files_dev", "resume_request_files_dev", "resume_check_files_dev", "file_windows_work_bytes",
           "put_response", "ack_offsets", "respond_window", "apply_acks", "respond_bytes_max", "respond_work_bytes",
           "apply_acks_work_bytes", "respond_files_dev", "apply_acks_files_dev", "PKT_DATA_ACK", "PKT_DATA_NAK",
           "NAK_REASON_GAP",
           "data_offsets", "OFFSET_IMPLIED", "OFFSET_NOT_DATA", "ValError"]
