"""GPU: the live audio history (include/emspec.h: emspec_set_live_audio, emspec_live_audio, emspec_audio_view*,
emspec_audio_batch*): a ring on the device of the samples the streaming calls were fed, views that read
a range back bit for bit, and a re-analysis of a held range at any fft size, hop and reassign setting.

The reference of a view is the samples the test itself fed (for a PCM session tests/pcm_ref.py's decoded views), compared as
uint32; what a ring holds after every call is tests/audio_ref.py's replay of the same calls.  A re-analysis is held against the
columns the session delivered, against emspec_batch_device over the host's copy of the same samples and against the oracle:
byte for byte in EXACT mode, within the live-against-batch bound of tests/test_gpu_live.py (8.7e-4 dB) in FAST mode.

Shapes: 3 streams, FFT 1024 / hop 256, 64 rows unless a form needs more (two / three bands: 64 rows each).  The multi-resolution
entry takes n_low 8192 or 16384 only, so the 4096 / 1024 two-band session runs through the band entry and the multi-resolution
entry at 8192 / 1024; the band entry takes sizes from 1024 up, so the three-band session is 4096 / 2048 / 1024."""
import numpy as np
import pytest

import audio_ref as A
import emspec
import oracle as O
import pcm_ref

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
N, HOP, S, R = 1024, 256, 3, 64
MODES = pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
TOL_DB = 8.7e-4                               # FAST mode, live against batch (tests/test_gpu_live.py)
NEG_ZERO = U(0x80000000)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """(tests/conftest.py: torch's HIP runtime is initialised before the first engine is created)"""
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()


def _engine(exact, rows=R, **kw):
    return emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST, rows=rows, **kw)


def _noise(streams, L, seed=3):
    return (np.random.default_rng(seed).standard_normal((streams, L)) * 0.2).astype(F)


def _patterns(L, seed=5):
    """Random 32-bit patterns as float32: exponents up to 2^1 (|x| < 4) kept, every larger one set to all ones with a non-zero
    mantissa (a NaN with the pattern's payload), and -0 at every 97th place."""
    u = np.random.default_rng(seed).integers(0, 1 << 32, L, dtype=np.uint64).astype(U)
    big = ((u >> U(23)) & U(0xFF)) > U(128)
    u[big] |= U(0x7F800001)
    u[::97] = NEG_ZERO
    assert np.isnan(u.view(F)).sum() > L // 4 and np.all(np.abs(u.view(F)[~np.isnan(u.view(F))]) <= 4.0)
    return u.view(F)


def _bits(x):
    return np.ascontiguousarray(x).view(U)


def _refused(code, call):
    with pytest.raises(emspec.EmspecError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


def _same_db(got, want, exact):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape
    if exact:
        assert np.array_equal(_bits(got), _bits(want))
    else:
        err = float(np.max(np.abs(got - want)))
        print("max |dB difference|", err)
        assert err < TOL_DB, err


def _check_held(e, model, fed, session="multi", pushed=None, n=N, hop=HOP):
    """live_audio is the model's held range for every stream, it trails what was pushed by less than a frame before the first
    frame and by less than a hop after, and a view of everything held is what was fed, bit for bit."""
    fed = _bits(fed)
    for s in range(model.S):
        held = e.live_audio(s, session)
        assert held == model.held(s), (s, held, model.held(s))
        end, first = held
        if pushed is not None:
            assert 0 <= pushed - end < (n if pushed < n else hop), (s, pushed, end)
    ends = {model.held(s) for s in range(model.S)}
    if len(ends) == 1:
        end, first = ends.pop()
        if end > first:
            got = e.audio_view(first, end - first, session=session)
            assert got.shape == (model.S, end - first)
            assert np.array_equal(_bits(got), fed[:, first:end])
            assert np.array_equal(_bits(got), model.view(first, end - first))


# ---- 1. bits ----
def test_bits_through_every_block_size_and_alignment():
    import torch
    Wb = 6001
    blocks = (128, 333, 4097, 3 * Wb + 5)
    L = sum(blocks)
    pcm = np.concatenate([_noise(2, L), _patterns(L)[None]])
    bits = _bits(pcm)
    with _engine(False) as e:
        assert e.live_audio(0) is None                     # no audio history
        e.set_live_audio(Wb)
        assert e.live_audio(0) is None and e.live_audio(0, "one") is None   # a session that has not started has no streams
        model = A.Session(S, N, HOP, Wb)
        a = 0
        for cnt in blocks:
            e.push_samples_multi(pcm, N, HOP, True, count=cnt, offset=a)
            model.push(pcm[:, a:a + cnt])
            a += cnt
            _check_held(e, model, pcm, pushed=a)
            end, first = e.live_audio(0)
            if end == 0:
                continue
            # one sample at either end; a range across the wrap; destinations 4, 8 and 12 bytes behind a 16-byte boundary with
            # a stride of count + 3, on the device and on the host: the samples, and nothing beside them
            ranges = [(first, 1), (end - 1, 1)]
            wrap = end // Wb * Wb
            if first < wrap - 5 and wrap + 6 <= end:
                ranges.append((wrap - 5, 11))
                ranges.append((first, end - first))
                assert first % Wb > 0 and (first % Wb) + (end - first) > Wb
            for va, vc in ranges:
                for off in (0, 1, 2, 3):
                    buf = torch.full((S * (vc + 3) + 8,), 12345.0, dtype=torch.float32, device="cuda")
                    assert buf.data_ptr() % 16 == 0
                    e.audio_view_device(va, vc, buf[off:], stride=vc + 3)
                    torch.cuda.synchronize()
                    got = buf.cpu().numpy()
                    rows = got[off:off + S * (vc + 3)].reshape(S, vc + 3)
                    assert np.array_equal(_bits(rows[:, :vc]), bits[:, va:va + vc]), (va, vc, off)
                    assert np.all(got[:off] == 12345.0) and np.all(rows[:-1, vc:] == 12345.0) and np.all(got[off + (S - 1) * (vc + 3) + vc:] == 12345.0)
                host = np.full((S, vc + 3), 12345.0, F)
                assert e.audio_view(va, vc, pcm=host, stride=vc + 3) is host
                assert np.array_equal(_bits(host[:, :vc]), bits[:, va:va + vc]) and np.all(host[:, vc:] == 12345.0)
                pin = emspec.PinnedArray((S, vc + 3), F)
                try:
                    pin.array[...] = 12345.0
                    e.audio_view(va, vc, pcm=pin.array, stride=vc + 3)
                    assert np.array_equal(_bits(pin.array[:, :vc]), bits[:, va:va + vc]) and np.all(pin.array[:, vc:] == 12345.0)
                finally:
                    pin.close()
            one = e.audio_view(end - 2, 2, stream0=2, streams=1)
            assert np.array_equal(_bits(one), bits[2:3, end - 2:end])
        # (the last block's last round completed frames, and a launch moves everything staged: nothing trails)
        assert e.live_audio(0) == model.held(0) == (L, L - Wb)
        assert model.launches == 3     # (the first two blocks only joined the staging block; the last took two rounds, the first of them more than W)
        assert np.isnan(e.audio_view(e.live_audio(2)[1], Wb, stream0=2)).sum() > Wb // 4   # (the NaNs came back as NaNs)


# ---- 2. every feeding form ----
@pytest.mark.parametrize("form", ["frame", "block", "one", "multires", "twoband", "multiband", "pcm"])
def test_every_form_holds_what_it_was_fed(form):
    Wf = 1500
    if form == "frame":
        D = emspec.latency_columns(N, HOP, True)
        pcm = _noise(S, N + 8 * HOP)
        with _engine(False) as e:
            e.set_live_audio(Wf)
            model = A.Session(S, N, HOP, Wf, form="frame")
            for j in range(9):
                frames = np.ascontiguousarray(pcm[:, j * HOP:j * HOP + N])
                _, _, cols = e.columns(frames, HOP, True)
                assert np.all(cols == (j - D if j >= D else -1))      # (the empty columns while priming store their samples too)
                model.frames(frames)
                _check_held(e, model, pcm)
                assert e.live_audio(0)[0] == j * HOP + N
            before = [e.live_audio(s) for s in range(S)]
            while True:                                               # flushes store nothing
                try:
                    e.columns_flush()
                except emspec.EmspecError as err:
                    assert err.code == emspec.ERR_STATE
                    break
                assert [e.live_audio(s) for s in range(S)] == before
            _check_held(e, model, pcm)
    elif form == "block":
        pcm = _noise(S, N + 9 * HOP + 77)
        with _engine(False) as e:
            e.set_live_audio(Wf)
            model = A.Session(S, N, HOP, Wf)
            for a in range(0, pcm.shape[1], 300):
                cnt = min(300, pcm.shape[1] - a)
                e.push_samples_multi(pcm, N, HOP, True, count=cnt, offset=a)
                model.push(pcm[:, a:a + cnt])
                _check_held(e, model, pcm, pushed=a + cnt)
            before = [e.live_audio(s) for s in range(S)]
            e.columns_flush()
            assert [e.live_audio(s) for s in range(S)] == before
            _check_held(e, model, pcm)
    elif form == "one":
        pcm = _noise(1, N + 9 * HOP + 77)
        with _engine(False) as e:
            e.set_live_audio(Wf)
            model = A.Session(1, N, HOP, Wf, form="frame")
            for j in range(6):
                e.column(pcm[0, j * HOP:j * HOP + N], HOP, True)
                model.frames(pcm[:, j * HOP:j * HOP + N])
                _check_held(e, model, pcm, session="one")
            assert e.live_audio(0, "multi") is None
            before = e.live_audio(0, "one")
            e.flush()
            assert e.live_audio(0, "one") == before
            e.reset()
            assert e.live_audio(0, "one") is None
            model = A.Session(1, N, HOP, Wf)
            for a in range(0, pcm.shape[1], 333):
                cnt = min(333, pcm.shape[1] - a)
                e.push_samples(pcm[0, a:a + cnt], N, HOP, True)
                model.push(pcm[:, a:a + cnt])
                _check_held(e, model, pcm, session="one", pushed=a + cnt)
    elif form in ("multires", "twoband", "multiband"):
        n0, rows = {"multires": (8192, 128), "twoband": (4096, 128), "multiband": (4096, 192)}[form]
        pcm = _noise(S, n0 + 6 * HOP + 5)
        with _engine(False, rows=rows) as e:
            e.set_live_audio(Wf)
            if form == "multires":
                feed = lambda a, cnt: e.push_samples_multires(pcm, 8192, 1024, HOP, 64, True, count=cnt, offset=a)
            elif form == "twoband":
                feed = lambda a, cnt: e.push_samples_multiband(pcm, (4096, 1024), (64,), HOP, True, count=cnt, offset=a)
            else:
                feed = lambda a, cnt: e.push_samples_multiband(pcm, (4096, 2048, 1024), (64, 128), HOP, True, count=cnt, offset=a)
            model = A.Session(S, n0, HOP, Wf)
            step = 5 * HOP + 3
            for a in range(0, pcm.shape[1], step):
                cnt = min(step, pcm.shape[1] - a)
                feed(a, cnt)
                model.push(pcm[:, a:a + cnt])
                _check_held(e, model, pcm, pushed=a + cnt, n=n0)
            assert e.live_audio(0)[0] > Wf
        if form == "multiband":      # the per-frame form of a band session
            with _engine(False, rows=128) as e:
                e.set_live_audio(Wf)
                model = A.Session(S, 4096, HOP, Wf, form="frame")
                for j in range(3):
                    frames = np.ascontiguousarray(pcm[:, j * HOP:j * HOP + 4096])
                    e.columns_multiband(frames, (4096, 1024), (64,), HOP, True)
                    model.frames(frames)
                    _check_held(e, model, pcm)
    else:
        rng = np.random.default_rng(9)
        frames = N + 9 * HOP + 77
        raw = rng.integers(0, 256, size=(2, frames * 4), dtype=np.uint8)          # s16 stereo, full range
        fmt = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", "side"])
        decoded = pcm_ref.decode(raw, pcm_ref.S16, 2, fmt.matrix)                 # [8][frames]: L R M S of either source
        typed = raw.view(fmt.dtype)
        with _engine(False) as e:
            e.set_live_audio(Wf)
            model = A.Session(8, N, HOP, Wf, pcm=True)
            for a in range(0, frames, 300):
                cnt = min(300, frames - a)
                e.push_samples_pcm(typed, fmt, N, HOP, True, count=cnt, offset=a)
                model.push(decoded[:, a:a + cnt])
                _check_held(e, model, decoded, pushed=a + cnt)
            assert e.live_streams == 8 and e.live_audio(7)[0] > Wf


# ---- 3. emspec_reset_stream, emspec_reset ----
def test_reset_stream_restarts_one_stream_and_reset_empties_all():
    Wf = 1500
    pcm = _noise(S, N + 12 * HOP)
    with _engine(False) as e:
        e.set_live_audio(Wf)
        model = A.Session(S, N, HOP, Wf)
        cut = N + 5 * HOP + 100
        e.push_samples_multi(pcm, N, HOP, True, count=cut, offset=0)
        model.push(pcm[:, :cut])
        _check_held(e, model, pcm, pushed=cut)
        before = [e.live_audio(s) for s in range(S)]
        e.reset_stream(1)
        model.reset_stream(1)
        assert e.live_audio(1) == (0, 0) and [e.live_audio(0), e.live_audio(2)] == [before[0], before[2]]
        _refused(emspec.ERR_INVALID_ARG, lambda: e.audio_view(0, 1, stream0=1, streams=1))
        for s in (0, 2):
            end, first = before[s]
            assert np.array_equal(_bits(e.audio_view(first, end - first, stream0=s, streams=1)), _bits(pcm)[s:s + 1, first:end])
        # the stream restarts its numbering: it is fed from the cut on, the others continue
        e.push_samples_multi(pcm, N, HOP, True, count=pcm.shape[1] - cut, offset=cut)
        model.push(pcm[:, cut:])
        for s in range(S):
            assert e.live_audio(s) == model.held(s)
        end, first = e.live_audio(1)
        assert 0 < end <= pcm.shape[1] - cut and first == max(0, end - Wf)
        assert np.array_equal(_bits(e.audio_view(first, end - first, stream0=1, streams=1)), _bits(pcm)[1:2, cut + first:cut + end])
        end, first = e.live_audio(0)
        assert np.array_equal(_bits(e.audio_view(first, end - first, stream0=0, streams=1)), _bits(pcm)[0:1, first:end])
        assert np.array_equal(_bits(e.audio_view(first, end - first, stream0=2, streams=1)), model.view(first, end - first, 2, 1))
        _refused(emspec.ERR_INVALID_ARG, lambda: e.audio_view(first, end - first))          # (stream 1 does not hold that range)
        e.reset()
        assert all(e.live_audio(s) is None for s in range(S))
        _refused(emspec.ERR_STATE, lambda: e.audio_view(0, 1))
        e.push_samples_multi(pcm, N, HOP, True, count=N, offset=0)
        assert e.live_audio(0) == (N, 0)
        assert np.array_equal(_bits(e.audio_view(0, N)), _bits(pcm)[:, :N])


# ---- 4. cleared is untouched ----
def _script(e, pcm, between=None):
    """Per-hop pushes, then the flushes -> every delivered column [S][columns][rows] and its RGBA."""
    dbs, rgbas = [], []
    for a in range(0, pcm.shape[1], HOP):
        db, rgba, counts, _ = e.push_samples_multi(pcm, N, HOP, True, want_rgba=True, count=min(HOP, pcm.shape[1] - a), offset=a)
        assert len(set(counts.tolist())) == 1
        dbs.append(db[:, :counts[0]].copy())
        rgbas.append(rgba[:, :counts[0]].copy())
        if between:
            between()
    while True:
        try:
            db, rgba, cols = e.columns_flush(want_rgba=True)
        except emspec.EmspecError as err:
            assert err.code == emspec.ERR_STATE
            break
        dbs.append(db[:, None].copy())
        rgbas.append(rgba[:, None].copy())
    return np.concatenate(dbs, axis=1), np.concatenate(rgbas, axis=1)


@MODES
def test_cleared_is_untouched(exact):
    import torch
    pcm = _noise(S, N + 19 * HOP)
    with _engine(exact) as e:
        never = _script(e, pcm)
    with _engine(exact) as e:
        e.set_live_audio(5000)
        e.push_samples_multi(pcm, N, HOP, True, count=N + HOP, offset=0)
        assert e.live_audio(0) == (N + HOP, 0)
        e.reset()
        e.set_live_audio(0)
        cleared = _script(e, pcm)
        assert e.live_audio(0) is None
        buf = torch.zeros((S, N), dtype=torch.float32, device="cuda")
        db = torch.zeros((S, 1, R), dtype=torch.float32, device="cuda")
        _refused(emspec.ERR_STATE, lambda: e.audio_view(0, N))
        _refused(emspec.ERR_STATE, lambda: e.audio_view_device(0, N, buf))
        _refused(emspec.ERR_STATE, lambda: e.audio_batch_device(0, N, N, HOP, db=db))
        _refused(emspec.ERR_STATE, lambda: e.audio_batch(0, N, N, HOP))
    assert never[0].shape == cleared[0].shape == (S, 20, R)
    _same_db(cleared[0], never[0], exact)
    if exact:
        assert np.array_equal(cleared[1], never[1])


# ---- 5. re-analysis ----
@MODES
def test_reanalysis_of_a_held_range(exact):
    import torch
    Wr, hops = 8192, 40
    L = N + (hops - 1) * HOP
    D = emspec.latency_columns(N, HOP, True)
    pcm = _noise(S, L)
    dev = lambda cols: torch.zeros((S, cols, R), dtype=torch.float32, device="cuda")
    with _engine(exact) as e:
        e.set_live_audio(Wr)
        delivered = []
        for a in range(0, L, HOP):
            db, _, counts, _ = e.push_samples_multi(pcm, N, HOP, True, count=min(HOP, L - a), offset=a)
            delivered.append(db[:, :counts[0]].copy())
        delivered = np.concatenate(delivered, axis=1)
        end, first = e.live_audio(0)
        assert (end, first) == (L, L - Wr) and first % HOP == 0 and delivered.shape[1] == hops - D
        j0, count = first // HOP, end - first
        # the session's own n / hop / reassign: the columns away from the range's ends are the session's
        C = emspec.num_columns(count, N, HOP)
        out = dev(C)
        e.audio_batch_device(first, count, N, HOP, True, db=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert C - 2 * D > 8 and j0 + C - D <= delivered.shape[1]
        _same_db(got[:, D:C - D], delivered[:, j0 + D:j0 + C - D], exact)
        # another analysis of the same samples: the batch over the host's copy of them, and the oracle
        held = np.ascontiguousarray(pcm[:, first:end])
        held_t = torch.from_numpy(held).cuda()
        for n2, hop2, re2 in ((256, 128, True), (N, HOP, False), (256, 128, False)):
            C2 = emspec.num_columns(count, n2, hop2)
            out, ref = dev(C2), dev(C2)
            idx = torch.zeros((S, C2, R), dtype=torch.uint8, device="cuda")
            e.audio_batch_device(first, count, n2, hop2, re2, db=out, index=idx)
            e.batch_device(held_t, n2, hop2, re2, db=ref)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            _same_db(got, ref.cpu().numpy(), exact)
            cfg = O.make_cfg(n2, hop2, re2, rows=R)
            odb = O.batch_exact(cfg, held, want=("db",))[0] if exact else O.batch_f32(cfg, held, want=("db",))[0]
            _same_db(got, odb, exact)
            host = e.audio_batch(first, count, n2, hop2, re2, want=("db", "index", "rgba"))
            assert np.array_equal(_bits(host["db"]), _bits(got)) if exact else np.max(np.abs(host["db"] - got)) < TOL_DB
            if exact:
                assert np.array_equal(host["index"], idx.cpu().numpy())
            assert host["rgba"].shape == (S, C2, R, 4)
        # a sub-range of two streams
        C3 = emspec.num_columns(4096, 256, 128)
        out, ref = dev(C3)[:2].contiguous(), dev(C3)[:2].contiguous()
        e.audio_batch_device(first + 512, 4096, 256, 128, True, stream0=1, streams=2, db=out)
        e.batch_device(held_t[1:, 512:512 + 4096].contiguous(), 256, 128, True, db=ref)
        torch.cuda.synchronize()
        _same_db(out.cpu().numpy(), ref.cpu().numpy(), exact)
        # with a time reduction the output is the batch's (the flushes store nothing: the range stays)
        while True:
            try:
                e.columns_flush()
            except emspec.EmspecError:
                break
        assert e.live_audio(0) == (end, first)
        e.set_time_reduce(4)
        Cr = emspec.reduced_columns(C, 4)
        out, ref = dev(Cr), dev(Cr)
        e.audio_batch_device(first, count, N, HOP, True, db=out)
        e.batch_device(held_t, N, HOP, True, db=ref)
        torch.cuda.synchronize()
        _same_db(out.cpu().numpy(), ref.cpu().numpy(), exact)
        host = e.audio_batch(first, count, N, HOP, True)["db"]
        assert host.shape == (S, Cr, R)
        _same_db(host, out.cpu().numpy(), exact)
        e.set_time_reduce(1)


# ---- 6. the session is not disturbed ----
def test_reanalysis_between_pushes_does_not_disturb_the_session():
    import torch
    pcm = _noise(S, N + 19 * HOP)
    with _engine(True) as e:
        plain = _script(e, pcm)
    with _engine(True) as e:
        e.set_live_audio(4096)
        ran = [0]

        def between():
            held = e.live_audio(0)
            if held is None or held[0] - held[1] < 256:
                return
            end, first = held
            cols = emspec.num_columns(end - first, 256, 128)
            out = torch.zeros((S, cols, R), dtype=torch.float32, device="cuda")
            e.audio_batch_device(first, end - first, 256, 128, False, db=out)
            e.audio_batch(first, end - first, 256, 128, True, want=("db", "rgba"))
            ran[0] += 1
        with_re = _script(e, pcm, between)
        assert ran[0] >= 15
    assert np.array_equal(_bits(with_re[0]), _bits(plain[0])) and np.array_equal(with_re[1], plain[1])


# ---- 7. with the other overlays ----
@MODES
def test_with_history_peaks_envelope_and_display(exact):
    k, Wh, Wa = 4, 6, 3000
    pcm = _noise(S, N + 14 * HOP)
    D = emspec.latency_columns(N, HOP, True)
    with _engine(exact) as e:
        e.set_display(0.5, 0.6)
        e.set_live_history(Wh)
        e.set_live_audio(Wa)
        pk = np.zeros((S, 1, k, 2), F)
        wv = np.zeros((S, 1, 2), F)
        e.set_live_peaks(k, -70.0, pk)
        e.set_live_wave(wv)
        model = A.Session(S, N, HOP, Wa)
        cols, pks, wvs = [], [], []
        for a in range(0, pcm.shape[1], HOP):
            db, _, counts, _ = e.push_samples_multi(pcm, N, HOP, True, count=HOP, offset=a)
            model.push(pcm[:, a:a + HOP])
            _check_held(e, model, pcm, pushed=a + HOP)
            if counts[0]:
                assert np.all(counts == 1)
                cols.append(db[:, 0].copy()); pks.append(pk[:, 0].copy()); wvs.append(wv[:, 0].copy())
        cols, pks, wvs = np.stack(cols, 1), np.stack(pks, 1), np.stack(wvs, 1)
        ncol = cols.shape[1]
        assert ncol == 15 - D
        # every overlay's own equality: the peaks are those of the delivered column, the envelope the samples' under it, the
        # history's newest columns the delivered ones - and the audio view is still what was fed
        assert np.array_equal(_bits(pks), _bits(emspec.peaks_host(cols, k, -70.0)))
        assert np.array_equal(_bits(wvs), _bits(emspec.wave_host(pcm, N, HOP)[:, :ncol]))
        assert e.live_history(0) == (ncol, ncol - Wh)
        assert np.array_equal(_bits(e.history_view(ncol - Wh, 1, Wh)["db"]), _bits(cols[:, ncol - Wh:]))
        end, first = e.live_audio(0)
        assert (end, first) == (pcm.shape[1], pcm.shape[1] - Wa)
        assert np.array_equal(_bits(e.audio_view(first, Wa)), _bits(pcm)[:, first:end])
        e.set_live_peaks(1, 0.0, None)
        e.set_live_wave(None)


# ---- 8. refusals leave the engine usable ----
def test_refusals_leave_the_engine_usable():
    import torch
    Wf = 2000
    pcm = _noise(S, N + 8 * HOP)
    with _engine(False) as e:
        _refused(emspec.ERR_INVALID_ARG, lambda: e.set_live_audio((1 << 28) + 1))
        _refused(emspec.ERR_INVALID_ARG, lambda: e.set_live_audio(-1))
        e.set_live_audio(Wf)
        e.push_samples_multi(pcm, N, HOP, True)
        end, first = e.live_audio(0)
        assert (end, first) == (pcm.shape[1], pcm.shape[1] - Wf)
        bits = _bits(pcm)
        buf = torch.zeros((S * Wf + 4,), dtype=torch.float32, device="cuda")
        db = torch.zeros((S, 8, R), dtype=torch.float32, device="cuda")
        lib, h = e._lib, e._h

        def ok():
            got = e.audio_view(first, Wf)
            assert np.array_equal(_bits(got), bits[:, first:end])
            assert e.live_audio(0) == (end, first)
        ok()
        cases = [
            lambda: e.audio_view(first - 1, 2),                                   # below the first held sample
            lambda: e.audio_view(end - 1, 2),                                     # past the end
            lambda: e.audio_view(end, 1),
            lambda: e.audio_view(first, 0),                                       # count = 0
            lambda: e.audio_view(first, 10, pcm=np.zeros((S, 9), F), stride=9),   # stride < count
            lambda: e.audio_view(first, 10, stream0=1, streams=3),                # streams outside the session
            lambda: e.audio_view(first, 10, stream0=-1, streams=1),
            lambda: e.audio_view(first, 10, stream0=0, streams=0),
            lambda: e.audio_view_device(first, 10, None),                         # NULL output
            lambda: e.audio_view_device(first - 1, 2, buf),
            lambda: e.audio_view_device(first, Wf + 1, buf, stride=Wf + 1),
            lambda: e.audio_batch_device(first, N - 1, N, HOP, db=db),            # count < n
            lambda: e.audio_batch_device(first, Wf, 1000, HOP, db=db),            # the batch's own refusal: fft size
            lambda: e.audio_batch_device(first - 1, N, N, HOP, db=db),
            lambda: e.audio_batch(first, N - 1, N, HOP),
        ]
        for i, call in enumerate(cases):
            msg = _refused(emspec.ERR_INVALID_ARG, call)
            if i in (0, 1, 2):
                assert "stream 0" in msg and "[%d, %d)" % (first, end) in msg, msg
            ok()
        # a device pointer that is not 4-byte aligned, and a NULL host output, through the C entry
        import ctypes as C
        assert lib.emspec_audio_view_device(h, 0, 0, S, first, 10, C.c_void_p(buf.data_ptr() + 2), 10, None) == emspec.ERR_INVALID_ARG
        ok()
        assert lib.emspec_audio_view(h, 0, 0, S, first, 10, None, 10) == emspec.ERR_INVALID_ARG
        ok()
        assert lib.emspec_audio_view(h, 7, 0, S, first, 10, C.c_void_p(buf.data_ptr()), 10) == emspec.ERR_STATE   # no such session
        assert lib.emspec_live_audio(h, 7, 0, None) == -1 and lib.emspec_live_audio(h, 0, S, None) == -1
        assert lib.emspec_live_audio(None, 0, 0, None) == -1
        _refused(emspec.ERR_STATE, lambda: e.audio_view(first, 10, session="one"))       # a session that has not started
        ok()
        # W > 0 while a session has samples; 0 always clears
        _refused(emspec.ERR_STATE, lambda: e.set_live_audio(Wf + 1))
        _refused(emspec.ERR_STATE, lambda: e.set_live_audio(Wf))
        ok()
        torch.cuda.synchronize()
        e.set_live_audio(0)
        assert e.live_audio(0) is None
        _refused(emspec.ERR_STATE, lambda: e.set_live_audio(Wf))                         # (the session still has samples fed)
        e.reset()
        e.set_live_audio(Wf)
        e.push_samples_multi(pcm, N, HOP, True, count=N, offset=0)
        assert np.array_equal(_bits(e.audio_view(0, N)), bits[:, :N])
