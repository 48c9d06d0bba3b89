'use strict';
/*
 * emspec — Node/Electron host side of the MI355X reassigned-spectrogram engine.
 *
 * Exposes the call the renderer already makes (BASELINE.json north_star):
 *
 *     computeSpectrogramColumn(audioFrame, fftSize, hop, reassign) -> Float32Array(rows) of dB
 *
 * plus engine management and the batched entry point for throughput runs
 * (SURVEY.md §8(b)).  All numeric work happens in libemspec (HIP, gfx950);
 * this file only marshals typed arrays through the N-API addon.  There is no
 * JS/CPU fallback: without the addon or without a gfx950 device the calls throw.
 */
const native = require('./emspec.node');

class Engine {
  /** config: {device, rows, sampleRate, fminHz, fmaxHz, gain, dbTop, dbRange, gateDb, powerFloor, exact, streams, timeReduce}
   *  exact: true = EMSPEC_MODE_EXACT (binary64 arithmetic, 64-bit fixed-point histogram; include/emspec.h)
   *  streams: S > 1 = a live multi-stream engine: computeSpectrogramColumns / pushSamplesMulti advance all S streams per
   *  call in ONE kernel launch; its frame / column blocks are page-locked (engine.frames, engine.columnsDb, ...), so the
   *  kernel reads and writes them in place
   *  timeReduce: f > 1 = the batch calls (computeColumns, computeColumnsPacked, computeColumnsMultires, their PCM and async
   *  forms) return ceil(columns / f) columns per stream, each the maximum of f consecutive finished columns (setTimeReduce) */
  constructor(config = {}) {
    this.rows = native.rows(config);
    this._h = native.create(config);
    this._db = new Float32Array(this.rows);
    this.streams = Math.max(1, config.streams | 0);
    this.columnIndex = new Float64Array(this.streams);   // per stream: index of the column the last call returned (-1: empty)
    if (config.timeReduce !== undefined && config.timeReduce !== 1) this.setTimeReduce(config.timeReduce);
  }

  /**
   * Time reduction of the batch calls (emspec_set_time_reduce; the zoomed-out overview of a recording): groups of `factor`
   * consecutive finished columns collapse into one by maximum, on the device - dB by value, palette index by value, RGBA =
   * colour map at the reduced index.  Every batch call then takes output arrays of S * reducedColumns(C, factor) * rows cells
   * (wire: S * wireBound(reducedColumns(C, factor), rows)) and returns that column count; column g covers the time of columns
   * g * factor .. of the full-rate picture.  1 = off.  The live calls throw while factor > 1; setting it throws while a live
   * session has columns pending.
   */
  setTimeReduce(factor) { native.setTimeReduce(this._h, factor | 0); }
  get timeReduce() { return native.timeReduce(this._h); }

  /**
   * Waveform envelope (emspec_set_wave_out; DESIGN.md §3.12): while set, computeColumns*, computeColumnsPacked,
   * computeColumnsPcm*, the multi-resolution batch and batchPeaks also write (lo, hi) of the samples under each delivered column
   * to `wave`: a Float32Array of streams x delivered columns x 2 values or more (streams = sources x views for PCM), lo and hi
   * with the samples' own bits.  null clears it.  The addon keeps the array alive until it is replaced, cleared or the engine
   * is destroyed.
   */
  setWaveOut(wave) { native.setWaveOut(this._h, wave === undefined ? null : wave); }

  /**
   * Level meters (emspec_set_level_out, emspec_set_cross_out; DESIGN.md §3.17): while set, every call that honours setWaveOut
   * also writes the level records of its streams to `level` (levelRecords(streams x delivered columns) or more), and the PCM
   * calls the cross records of views a and b of each source to `cross` (crossRecords(sources x delivered columns) or more).
   * The records are exact integer sums, the same bytes whatever the mode; levelValues / crossCorrelation read them.  null
   * clears.  While setCrossOut is set, the calls on float streams throw EMSPEC_ERR_STATE.
   */
  setLevelOut(level) { native.setLevelOut(this._h, level ? level.bytes : null); }
  setCrossOut(a, b, cross) { native.setCrossOut(this._h, a | 0, b | 0, cross ? cross.bytes : null); }

  /**
   * Overlays of the live calls (emspec_set_live_peaks / emspec_set_live_wave; DESIGN.md §4.15): while set, every live call of
   * this engine also fills engine.columnsPeaks - Float32Array of (pos, dB) pairs, [(s * cols + slot) * k + i] - and
   * engine.columnsWave - (lo, hi) pairs, [s * cols + slot] - for exactly the column slots it writes: cols = 1 for
   * computeSpectrogramColumn(s) and the flushes, the call's maxColumns for the push calls.  Both are page-locked and sized like
   * engine.columnsDb, for `columns` columns per stream (default 1: one hop per call; a push that may complete more needs
   * {columns} at least its maxColumns, or it throws EMSPEC_ERR_INVALID_ARG).  The peaks are peaksOf(the delivered dB, k, minDb),
   * written also when only RGBA is taken; the envelope is waveOf(the samples fed) column by column, and can only be switched on
   * before a session's first frame (or after reset()).  null / false clears.
   */
  setLivePeaks(opts) {
    if (!opts) { native.setLivePeaks(this._h, 0, 0, null); this.columnsPeaks = undefined; return; }
    const k = opts.k === undefined ? 8 : opts.k | 0, minDb = opts.minDb === undefined ? -60 : +opts.minDb;
    const cols = Math.max(1, opts.columns | 0);
    const arr = new Float32Array(native.allocPinned(8 * this.streams * cols * Math.max(k, 1)));
    native.setLivePeaks(this._h, k, minDb, arr);
    this.columnsPeaks = arr;
  }
  setLiveWave(opts) {
    if (!opts) { native.setLiveWave(this._h, null); this.columnsWave = undefined; return; }
    const cols = Math.max(1, (opts === true ? 1 : opts.columns) | 0);
    const arr = new Float32Array(native.allocPinned(8 * this.streams * cols));
    native.setLiveWave(this._h, arr);
    this.columnsWave = arr;
  }

  /**
   * Live level meters (emspec_set_live_level / emspec_set_live_cross; DESIGN.md §3.17, §4.15): while set, every live call also
   * fills engine.columnsLevel - a levelRecords block, record [s * cols + slot] - and engine.columnsCross - a crossRecords block,
   * record [p * cols + slot] of pair p = streams p * views + a and p * views + b - for the column slots it writes, from the
   * samples under each column: exact sums, the same bytes as levelsOf / crossOf of the samples fed.  Page-locked, sized for
   * `columns` columns per stream (default 1), switched on before a session's first frame (or after reset()) like the envelope;
   * levelValues / crossCorrelation / levelSum / crossSum read them.  While the cross is set, resetStream throws
   * EMSPEC_ERR_STATE (a pair's streams restart together), and the engine's streams must be a multiple of `views`.
   * null / false clears.
   */
  setLiveLevel(opts) {
    if (!opts) { native.setLiveLevel(this._h, null); this.columnsLevel = undefined; return; }
    const count = this.streams * Math.max(1, (opts === true ? 1 : opts.columns) | 0);
    const rec = levelRecords(count, native.allocPinned(24 * count));
    native.setLiveLevel(this._h, rec.bytes);
    this.columnsLevel = rec;
  }
  setLiveCross(views, a, b, opts = true) {
    if (!opts || views === null || views === false) { native.setLiveCross(this._h, 0, 0, 0, null); this.columnsCross = undefined; return; }
    const pairs = views >= 1 ? Math.floor(this.streams / views) : 0;
    const count = Math.max(1, pairs) * Math.max(1, (opts === true ? 1 : opts.columns) | 0);
    const rec = crossRecords(count, native.allocPinned(16 * count));
    native.setLiveCross(this._h, views | 0, a | 0, b | 0, rec.bytes);
    this.columnsCross = rec;
  }

  /**
   * Live history (emspec_set_live_history / emspec_live_history / emspec_history_view, DESIGN.md §3.14): the engine keeps the
   * last `columns` dB columns every live call delivers, per stream, on the device; historyView reads them back reduced in time
   * and coloured - what a renderer needs when the scroll speed, the window, the dB range, the gain, the gate or the colour map
   * changes, or the user scrolls back.  Set it before a session's first frame (or after reset()); 0 clears.
   * liveHistory(stream) -> {end, first}: the columns the stream has emitted and the first one still held, or null.
   * historyView({stream0 = 0, streams = all from stream0, firstColumn, factor = 1, groups, map, want = ['db']}) ->
   *   {db: Float32Array(streams * groups * rows), index: Uint8Array, rgba: Uint8Array(x 4)} (those named in `want`): group g
   *   is the peak hold of columns firstColumn + g * factor ... of each stream; map = {dbTop, dbRange, gateDb, shiftDb} is the
   *   colour law of index / rgba (default: the engine's configuration, no shift).  A single-stream engine views the session of
   *   computeSpectrogramColumn / pushSamples.
   */
  setLiveHistory(columns) { native.setLiveHistory(this._h, columns); }
  _historySession() { return this.streams > 1 ? 0 : 1; }
  liveHistory(stream = 0) {
    const r = native.liveHistory(this._h, this._historySession(), stream);
    return r ? { end: r[0], first: r[1] } : null;
  }
  historyView(opts) {
    const stream0 = opts.stream0 | 0, streams = opts.streams === undefined ? this.streams - stream0 : opts.streams | 0;
    const groups = +opts.groups, factor = opts.factor === undefined ? 1 : opts.factor | 0;
    const want = opts.want || ['db'];
    const cells = Math.max(0, streams) * Math.max(0, groups) * this.rows;
    const out = {};
    if (want.includes('db')) out.db = new Float32Array(cells);
    if (want.includes('index')) out.index = new Uint8Array(cells);
    if (want.includes('rgba')) out.rgba = new Uint8Array(4 * cells);
    const m = opts.map ? Float32Array.of(opts.map.dbTop, opts.map.dbRange, opts.map.gateDb, opts.map.shiftDb || 0) : null;
    native.historyView(this._h, this._historySession(), stream0, streams, +opts.firstColumn, factor, groups, m,
      out.db || null, out.index || null, out.rgba || null);
    return out;
  }

  /**
   * Stereo image (emspec_set_stereo_colormap / emspec_batch_pcm_stereo / emspec_history_view_stereo, DESIGN.md §3.16): level and
   * balance of a channel pair in ONE picture, composed on the device - brightness from the louder channel's dB, hue from the
   * difference of the two.  A pair is two views of one source: a, b index format.views (['left', 'right']: a = 0, b = 1;
   * ['left', 'right', 'mid', 'side'] with a = 2, b = 3 is a width display).  map = {dbTop, dbRange, gateDb, shiftDb,
   * panRangeDb = 12} (default: the engine's configuration); want: any of 'level' (Float32Array, dB of the louder channel),
   * 'index', 'pan' (Uint8Array; pan 0 = all a .. 16 = centre .. 32 = all b), 'rgba' (Uint8Array x 4 = palette[pan][index]).
   * setStereoColormap(palette): Uint8Array(33 * 1024), e.g. makeStereoColormap(brightness); a new engine holds that of 0.5.
   * computeStereo(src, sources, frames, format, fftSize, hop, reassign, {a = 0, b = 1, map, want = ['index', 'pan']}) ->
   *   {columns, level, index, pan, rgba}: arrays of sources * columns * rows cells.  Only what is asked for crosses PCIe on the
   *   way out.  Throws EMSPEC_ERR_STATE while timeReduce > 1.
   * historyViewStereo({stream0 = 0, views = 2, pairs = all from stream0, a = 0, b = 1, firstColumn, factor = 1, groups, map,
   *   want = ['index', 'pan']}) -> the same of the live history's groups (see historyView), pairs * groups * rows cells: what a
   *   live stereo view redraws from.
   */
  setStereoColormap(palette) { native.setStereoColormap(this._h, palette); }
  _stereoOut(want, cells) {
    const out = {};
    if (want.includes('level')) out.level = new Float32Array(cells);
    if (want.includes('index')) out.index = new Uint8Array(cells);
    if (want.includes('pan')) out.pan = new Uint8Array(cells);
    if (want.includes('rgba')) out.rgba = new Uint8Array(4 * cells);
    return out;
  }
  computeStereo(src, sources, frames, format, fftSize, hop, reassign = true, opts = {}) {
    if (src.byteLength !== sources * frames * format.frameBytes) throw Object.assign(new Error('src must hold sources * frames frames'), { code: 'EMSPEC_ERR_INVALID_ARG' });
    const C = Math.max(0, native.numColumns(frames, fftSize, hop));
    const out = this._stereoOut(opts.want || ['index', 'pan'], Math.max(0, sources) * C * this.rows);
    out.columns = native.batchPcmStereo(this._h, src, format.sampleType, format.channels, format.views, format.mix, sources, fftSize, hop,
      !!reassign, opts.a === undefined ? 0 : opts.a | 0, opts.b === undefined ? 1 : opts.b | 0, stereoMap(opts.map),
      out.level || null, out.index || null, out.pan || null, out.rgba || null);
    return out;
  }
  historyViewStereo(opts) {
    const stream0 = opts.stream0 | 0, views = opts.views === undefined ? 2 : opts.views | 0;
    const pairs = opts.pairs === undefined ? Math.floor((this.streams - stream0) / Math.max(views, 1)) : opts.pairs | 0;
    const groups = +opts.groups, factor = opts.factor === undefined ? 1 : opts.factor | 0;
    const out = this._stereoOut(opts.want || ['index', 'pan'], Math.max(0, pairs) * Math.max(0, groups) * this.rows);
    native.historyViewStereo(this._h, this._historySession(), stream0, pairs, views, opts.a === undefined ? 0 : opts.a | 0,
      opts.b === undefined ? 1 : opts.b | 0, +opts.firstColumn, factor, groups, stereoMap(opts.map),
      out.level || null, out.index || null, out.pan || null, out.rgba || null);
    return out;
  }

  /**
   * Live audio history (emspec_set_live_audio / emspec_live_audio / emspec_audio_view / emspec_audio_batch, DESIGN.md §3.15):
   * the engine keeps the last `samples` samples every live call was fed, per stream, on the device - what a renderer needs when
   * FFT Size, Smoothing or Enhanced / Natural changes and the scroll-back image has to be computed again (Frequency Scale and
   * Low-End Boost: INTEGRATION.md).  Set it before a session's first samples (or after reset()); 0 clears.
   * liveAudio(stream) -> {end, first}: the samples of the stream that were stored and the first one still held, or null.
   * audioView({stream0 = 0, streams = all from stream0, firstSample, count}) -> Float32Array(streams * count), bit for bit.
   * reanalyse({stream0, streams, firstSample, count, fftSize, hop, reassign = true, want = ['db']}) ->
   *   {columns, db: Float32Array(streams * columns * rows), rgba: Uint8Array(x 4), index: Uint8Array} (those named in `want`):
   *   computeColumns of the held samples, at any fftSize / hop / reassign; honours setTimeReduce and the display settings.
   * A single-stream engine addresses the session of computeSpectrogramColumn / pushSamples.
   */
  setLiveAudio(samples) { native.setLiveAudio(this._h, samples); }
  liveAudio(stream = 0) {
    const r = native.liveAudio(this._h, this._historySession(), stream);
    return r ? { end: r[0], first: r[1] } : null;
  }
  audioView(opts) {
    const stream0 = opts.stream0 | 0, streams = opts.streams === undefined ? this.streams - stream0 : opts.streams | 0;
    const count = +opts.count;
    const out = new Float32Array(Math.max(0, streams) * Math.max(0, count));
    native.audioView(this._h, this._historySession(), stream0, streams, +opts.firstSample, count, out);
    return out;
  }
  reanalyse(opts) {
    const stream0 = opts.stream0 | 0, streams = opts.streams === undefined ? this.streams - stream0 : opts.streams | 0;
    const count = +opts.count, want = opts.want || ['db'];
    const full = Math.max(0, native.numColumns(count, opts.fftSize | 0, opts.hop | 0));
    const columns = Math.max(0, native.reducedColumns(full, this.timeReduce));
    const cells = Math.max(0, streams) * columns * this.rows;
    const out = { columns };
    if (want.includes('db')) out.db = new Float32Array(cells);
    if (want.includes('rgba')) out.rgba = new Uint8Array(4 * cells);
    if (want.includes('index')) out.index = new Uint8Array(cells);
    native.audioBatch(this._h, opts.session === undefined ? this._historySession() : opts.session | 0, stream0, streams, +opts.firstSample,
      count, opts.fftSize | 0, opts.hop | 0, opts.reassign === undefined ? true : !!opts.reassign, out.db || null, out.rgba || null,
      out.index || null);
    return out;
  }

  /** Page-locked Float32Array / Uint8Array views for the live calls, (re)made when the shape changes. */
  _liveBlocks(fftSize, wantRgba) {
    const S = this.streams, R = this.rows;
    if (fftSize > 0 && (!this.frames || this.frames.length !== S * fftSize)) this.frames = new Float32Array(native.allocPinned(4 * S * fftSize));
    if (!this.columnsDb) this.columnsDb = new Float32Array(native.allocPinned(4 * S * R));
    if (wantRgba && !this.columnsRgba) this.columnsRgba = new Uint8Array(native.allocPinned(4 * S * R));
  }

  /**
   * The live multi-stream form of computeSpectrogramColumn: one frame of each of the engine's S streams in, one finished
   * column of each out, ONE launch (emspec_columns).  frames: Float32Array(S * fftSize), stream after stream - pass
   * engine.frames (page-locked, filled by the caller) to avoid a staging copy; any Float32Array works.
   * Returns engine.columnsDb: Float32Array(S * rows) of dB (page-locked, overwritten by the next call); with wantRgba,
   * engine.columnsRgba holds the colours.  engine.columnIndex[s] = index of stream s's column, -1 while its ring primes.
   */
  computeSpectrogramColumns(frames, fftSize, hop, reassign = true, wantRgba = false) {
    this._liveBlocks(fftSize, wantRgba);
    native.columns(this._h, frames, this.streams, fftSize, hop, !!reassign, this.columnsDb, wantRgba ? this.columnsRgba : undefined,
      this.columnIndex);
    return this.columnsDb;
  }

  /** computeSpectrogramColumns off the JS thread (libuv pool): resolves with engine.columnsDb.  Do not touch the blocks or
   *  this engine until the promise settles. */
  computeSpectrogramColumnsAsync(frames, fftSize, hop, reassign = true, wantRgba = false) {
    this._liveBlocks(fftSize, wantRgba);
    return native.columnsAsync(this._h, frames, this.streams, fftSize, hop, !!reassign, this.columnsDb,
      wantRgba ? this.columnsRgba : undefined, this.columnIndex).then(() => this.columnsDb);
  }

  /** Every stream that still has pending columns emits its next one (others: the empty column, columnIndex -1);
   *  throws EMSPEC_ERR_STATE when no stream has any.  Returns engine.columnsDb. */
  flushColumns(wantRgba = false) {
    this._liveBlocks(0, wantRgba);   // (the column blocks only: a session fed by sample blocks never made a frame block)
    native.columnsFlush(this._h, this.columnsDb, wantRgba ? this.columnsRgba : undefined, this.columnIndex);
    return this.columnsDb;
  }

  /**
   * Live streaming by sample blocks for all S streams (emspec_push_samples_multi): samples = Float32Array(S * count),
   * `count` new samples of every stream, stream after stream (engine.sampleBlock(count) is a page-locked one).
   * Returns { maxColumns, counts, first, db, rgba }: stream s completed counts[s] columns,
   * db.subarray((s * maxColumns + i) * rows, ...) is its i-th, first[s] the absolute index of its first (-1 if none).
   * db / rgba / counts / first are engine-owned page-locked blocks, overwritten by the next call (copy what you keep).
   * Drain the pending columns with flushColumns().
   */
  pushSamplesMulti(samples, fftSize, hop, reassign = true, wantRgba = false) {
    const S = this.streams, count = samples.length / S;
    const maxColumns = native.pushColumnsMulti(this._h, count, fftSize, hop, !!reassign);
    let o = this._push;
    if (!o || o.maxColumns < maxColumns || (wantRgba && !o.rgbaAll)) {
      const cap = Math.max(maxColumns, 1);
      o = this._push = { maxColumns: cap, dbAll: new Float32Array(native.allocPinned(4 * S * cap * this.rows)),
        rgbaAll: wantRgba ? new Uint8Array(native.allocPinned(4 * S * cap * this.rows)) : undefined,
        counts: new Float64Array(S), first: new Float64Array(S) };
    }
    native.pushMulti(this._h, samples, S, fftSize, hop, !!reassign, o.maxColumns, o.dbAll, wantRgba ? o.rgbaAll : undefined, o.counts, o.first);
    return { maxColumns: o.maxColumns, counts: o.counts, first: o.first, db: o.dbAll, rgba: wantRgba ? o.rgbaAll : undefined };
  }

  /**
   * The live calls' multi-resolution form (emspec_columns_multires / emspec_push_samples_multires, DESIGN.md §3.8): the image
   * of computeColumnsMultires column by column - opts.lowFftSize below the split, opts.fftSize from it up, one column per hop
   * at the latency of lowFftSize.  opts as in computeColumnsMultires ({fftSize, lowFftSize, hop, splitHz | splitRow,
   * reassign = true}) plus wantRgba.  frames: Float32Array(S * lowFftSize).  Results, flushColumns() and resetStream() as for
   * computeSpectrogramColumns; a session is one kind or the other until reset().
   */
  computeSpectrogramColumnsMultires(frames, opts) {
    const m = this._multiresOpts(opts);
    this._liveBlocks(opts.lowFftSize, m.wantRgba);
    native.columns(this._h, frames, this.streams, opts.lowFftSize, opts.hop, m.reassign, this.columnsDb,
      m.wantRgba ? this.columnsRgba : undefined, this.columnIndex, opts.fftSize, m.split);
    return this.columnsDb;
  }

  /** pushSamplesMulti for a multi-resolution session: same return value, opts as in computeSpectrogramColumnsMultires. */
  pushSamplesMultires(samples, opts) {
    const m = this._multiresOpts(opts);
    const S = this.streams, count = samples.length / S;
    const maxColumns = native.pushColumnsMulti(this._h, count, opts.lowFftSize, opts.hop, m.reassign, opts.fftSize);
    let o = this._push;
    if (!o || o.maxColumns < maxColumns || (m.wantRgba && !o.rgbaAll)) {
      const cap = Math.max(maxColumns, 1);
      o = this._push = { maxColumns: cap, dbAll: new Float32Array(native.allocPinned(4 * S * cap * this.rows)),
        rgbaAll: m.wantRgba ? new Uint8Array(native.allocPinned(4 * S * cap * this.rows)) : undefined,
        counts: new Float64Array(S), first: new Float64Array(S) };
    }
    native.pushMulti(this._h, samples, S, opts.lowFftSize, opts.hop, m.reassign, o.maxColumns, o.dbAll,
      m.wantRgba ? o.rgbaAll : undefined, o.counts, o.first, opts.fftSize, m.split);
    return { maxColumns: o.maxColumns, counts: o.counts, first: o.first, db: o.dbAll, rgba: m.wantRgba ? o.rgbaAll : undefined };
  }

  /**
   * The live calls' multi-band form (emspec_columns_multiband / emspec_push_samples_multiband, DESIGN.md §3.13): the image of
   * computeColumnsMultiband column by column, one column per hop at the latency of fftSizes[0].  opts as computeColumnsMultiband
   * takes them ({fftSizes, hop, splitHz | splitRows, reassign = true}) plus wantRgba.  frames: Float32Array(S * fftSizes[0]).
   * Results, flushColumns() and resetStream() as for computeSpectrogramColumns; a session is one kind until reset().
   */
  computeSpectrogramColumnsMultiband(frames, opts) {
    const m = this._multibandOpts(opts);
    this._liveBlocks(m.sizes[0], m.wantRgba);
    native.columns(this._h, frames, this.streams, m.sizes[0], opts.hop, m.reassign, this.columnsDb,
      m.wantRgba ? this.columnsRgba : undefined, this.columnIndex, 0, 0, m.sizes, m.splits);
    return this.columnsDb;
  }

  /** pushSamplesMulti for a multi-band session: same return value, opts as in computeSpectrogramColumnsMultiband. */
  pushSamplesMultiband(samples, opts) {
    const m = this._multibandOpts(opts);
    const S = this.streams, count = samples.length / S;
    const o = this._pushBlocks(native.pushColumnsMulti(this._h, count, m.sizes[0], opts.hop, m.reassign, 0, m.sizes), m.wantRgba);
    native.pushMulti(this._h, samples, S, m.sizes[0], opts.hop, m.reassign, o.maxColumns, o.dbAll,
      m.wantRgba ? o.rgbaAll : undefined, o.counts, o.first, 0, 0, m.sizes, m.splits);
    return { maxColumns: o.maxColumns, counts: o.counts, first: o.first, db: o.dbAll, rgba: m.wantRgba ? o.rgbaAll : undefined };
  }

  /** pushSamplesPcm for a multi-band session (emspec_push_samples_pcm_multiband): block and format as there, opts as above. */
  pushSamplesPcmMultiband(block, format, opts) {
    const m = this._multibandOpts(opts);
    const S = this.streams, sources = S / format.views;
    const count = block.byteLength / (sources * format.frameBytes);
    const o = this._pushBlocks(native.pushColumnsMulti(this._h, count, m.sizes[0], opts.hop, m.reassign, 0, m.sizes), m.wantRgba);
    native.pushPcm(this._h, block, format.sampleType, format.channels, format.views, format.mix, sources, m.sizes[0], opts.hop,
      m.reassign, o.maxColumns, o.dbAll, m.wantRgba ? o.rgbaAll : undefined, o.counts, o.first, 0, 0, m.sizes, m.splits);
    return { maxColumns: o.maxColumns, counts: o.counts, first: o.first, db: o.dbAll, rgba: m.wantRgba ? o.rgbaAll : undefined };
  }

  /** the push calls' engine-owned page-locked blocks, grown to hold maxColumns columns per stream */
  _pushBlocks(maxColumns, wantRgba) {
    const S = this.streams;
    let o = this._push;
    if (!o || o.maxColumns < maxColumns || (wantRgba && !o.rgbaAll)) {
      const cap = Math.max(maxColumns, 1);
      o = this._push = { maxColumns: cap, dbAll: new Float32Array(native.allocPinned(4 * S * cap * this.rows)),
        rgbaAll: wantRgba ? new Uint8Array(native.allocPinned(4 * S * cap * this.rows)) : undefined,
        counts: new Float64Array(S), first: new Float64Array(S) };
    }
    return o;
  }

  /** (the split rows of opts.splitHz are looked up once per list of frequencies, not per call) */
  _multibandOpts(opts) {
    let splits = opts.splitRows;
    if (splits === undefined) {
      const key = Array.from(opts.splitHz).join();
      if (this._mbHz !== key) { this._mbSplits = Array.from(opts.splitHz, (hz) => this.splitRowForHz(hz)); this._mbHz = key; }
      splits = this._mbSplits;
    }
    return { sizes: Int32Array.from(opts.fftSizes), splits: Int32Array.from(splits),
      reassign: opts.reassign === undefined ? true : !!opts.reassign, wantRgba: !!opts.wantRgba };
  }

  /**
   * Live session from raw interleaved frames (emspec_push_samples_pcm / _pcm_multires): the capture buffer in, the columns of
   * sources * format.views streams out (stream = source * views + view; sources = engine.streams / format.views).
   * block: `count` frames of every source, source after source, in the typed array of format.type (Int16Array, Int32Array,
   * Float32Array; Uint8Array for s24) - another element type throws EMSPEC_ERR_INVALID_ARG.  opts: {fftSize, hop, reassign =
   * true, wantRgba}; with fftSizeHigh + splitRow | splitHz the session is the multi-resolution one (fftSize is then the LOW
   * band's size, as lowFftSize in pushSamplesMultires).  Returns what pushSamplesMulti returns; flushColumns(),
   * resetStream(s) and reset() act as on any session.  A float live call on a PCM session (or the reverse), or another format
   * mid-session, throws EMSPEC_ERR_STATE until reset().
   */
  pushSamplesPcm(block, format, opts) {
    const S = this.streams, sources = S / format.views;
    const high = opts.fftSizeHigh | 0;
    const m = high ? this._multiresOpts(opts) : { split: 0, reassign: opts.reassign === undefined ? true : !!opts.reassign, wantRgba: !!opts.wantRgba };
    const count = block.byteLength / (sources * format.frameBytes);
    const maxColumns = high ? native.pushColumnsMulti(this._h, count, opts.fftSize, opts.hop, m.reassign, high)
      : native.pushColumnsMulti(this._h, count, opts.fftSize, opts.hop, m.reassign);
    let o = this._push;
    if (!o || o.maxColumns < maxColumns || (m.wantRgba && !o.rgbaAll)) {
      const cap = Math.max(maxColumns, 1);
      o = this._push = { maxColumns: cap, dbAll: new Float32Array(native.allocPinned(4 * S * cap * this.rows)),
        rgbaAll: m.wantRgba ? new Uint8Array(native.allocPinned(4 * S * cap * this.rows)) : undefined,
        counts: new Float64Array(S), first: new Float64Array(S) };
    }
    native.pushPcm(this._h, block, format.sampleType, format.channels, format.views, format.mix, sources, opts.fftSize, opts.hop,
      m.reassign, o.maxColumns, o.dbAll, m.wantRgba ? o.rgbaAll : undefined, o.counts, o.first, high, m.split);
    return { maxColumns: o.maxColumns, counts: o.counts, first: o.first, db: o.dbAll, rgba: m.wantRgba ? o.rgbaAll : undefined };
  }

  /** (the split row of opts.splitHz is looked up once per frequency, not per call) */
  _multiresOpts(opts) {
    let split = opts.splitRow;
    if (split === undefined) {
      if (this._mrHz !== opts.splitHz) { this._mrSplit = this.splitRowForHz(opts.splitHz); this._mrHz = opts.splitHz; }
      split = this._mrSplit;
    }
    return { split, reassign: opts.reassign === undefined ? true : !!opts.reassign, wantRgba: !!opts.wantRgba };
  }

  /** A page-locked Float32Array(S * count) for pushSamplesMulti (kept per count). */
  sampleBlock(count) {
    if (!this._blk || this._blk.length !== this.streams * count) this._blk = new Float32Array(native.allocPinned(4 * this.streams * count));
    return this._blk;
  }

  /** Restart stream s of the live session (its position, pending columns, display state); the others continue. */
  resetStream(s) { native.resetStream(this._h, s); }

  /**
   * One frame in, one finished column out.  With time reassignment on, the column
   * returned for call j is column j - latencyColumns(fftSize, hop) (energy can move
   * that many columns either way); the first calls return the empty column and set
   * engine.lastColumn = -1.  Returns a Float32Array(rows) of dB owned by the caller.
   */
  computeSpectrogramColumn(audioFrame, fftSize, hop, reassign = true, outRgba = undefined) {
    const out = new Float32Array(this.rows);
    this.lastColumn = native.column(this._h, audioFrame, fftSize, hop, !!reassign, out, outRgba);
    return out;
  }

  /**
   * Streaming by sample blocks (what an audio callback delivers): feed any number of new samples; every
   * `hop` of them completes a frame.  Returns { first, count, db, rgba }: `count` finished columns,
   * oldest first, `first` = absolute index of the first (-1 when count is 0), db = Float32Array(count*rows),
   * rgba = Uint8Array(4*count*rows) when wantRgba.  Drain the last D columns with flush().
   */
  pushSamples(samples, fftSize, hop, reassign = true, wantRgba = false) {
    const count = native.pushColumns(this._h, samples.length, fftSize, hop, !!reassign);
    const db = new Float32Array(count * this.rows);
    const rgba = wantRgba ? new Uint8Array(4 * count * this.rows) : undefined;
    const first = native.push(this._h, samples, fftSize, hop, !!reassign, this.rows, db, rgba);
    if (count > 0) this.lastColumn = first + count - 1;
    return { first, count, db, rgba };
  }

  /** Emit one of the columns still pending after the last frame; throws EMSPEC_ERR_STATE when none. */
  flush(outRgba = undefined) {
    const out = new Float32Array(this.rows);
    this.lastColumn = native.flush(this._h, out, outRgba);
    return out;
  }

  /**
   * Batched: pcm = Float32Array(S*L) (S streams of L samples, row-major) ->
   * out.db Float32Array(S*C*rows) and/or out.rgba Uint8Array(4*S*C*rows) and/or out.index Uint8Array(S*C*rows).
   * Returns C, the columns per stream.
   */
  computeColumns(pcm, S, L, fftSize, hop, reassign, out) {
    return native.batch(this._h, pcm, S, L, fftSize, hop, !!reassign, out.db, out.rgba, out.index);
  }

  /**
   * Spectral peaks (emspec_batch_peaks; include/emspec.h): pcm = Float32Array(S*L), S streams -> Float32Array laid out
   * [S][C][k][2]: per column the k (1..32, default 8) loudest local maxima at or above minDb (default -60), loudest first, each
   * as (position in row units, dB); unused slots are (-1, -Infinity).  Computed on the device from the dB columns computeColumns
   * would return; only the lists cross PCIe on the way out (64 bytes per column at k = 8 instead of 4 * rows).  positionToHz maps
   * a position to Hz, noteOf the Hz to a note.  Throws EMSPEC_ERR_STATE while timeReduce > 1.
   */
  computePeaks(pcm, streams, fftSize, hop, reassign, opts = {}) {
    const k = opts.k === undefined ? 8 : opts.k | 0, minDb = opts.minDb === undefined ? -60 : +opts.minDb;
    const L = Math.floor(pcm.length / streams);
    const C = Math.max(0, native.numColumns(L, fftSize, hop));
    const out = new Float32Array(streams * C * Math.min(32, Math.max(1, k)) * 2);
    native.batchPeaks(this._h, pcm, streams, L, fftSize, hop, !!reassign, k, minDb, out);
    return out;
  }
  /** A peak's position in row units -> Hz on this engine's row axis (emspec_position_hz): log-interpolated inside the row. */
  positionToHz(pos) { return native.positionHz(this._h, pos); }

  /**
   * Throughput entry with the palette-index columns kept compressed across PCIe (emspec_batch_packed): one lossless wire
   * image per stream, ~186 B instead of 1,024 B per column on typical audio.  wire: Uint8Array (allocPinned for full
   * speed; S * wireBound(C, rows) always suffices), offsets: Float64Array(S + 1).  Stream s is
   * wire.subarray(offsets[s], offsets[s + 1]); expand it on the host with unpackWire(image, C, rows, out) or keep /
   * forward it as it is.  Returns C, the columns per stream.
   */
  computeColumnsPacked(pcm, S, L, fftSize, hop, reassign, wire, offsets) {
    return native.batchPacked(this._h, pcm, S, L, fftSize, hop, !!reassign, wire, offsets);
  }

  /**
   * computeColumns from raw interleaved frames (emspec_batch_pcm): src = `sources` recordings of `frames` frames each, in the
   * typed array of format.type (see pcmFormat); out as in computeColumns, for sources * format.views streams (stream = source *
   * views + view).  The raw bytes cross PCIe; one kernel on the device converts and mixes them (DESIGN.md §3.9).  Returns C.
   */
  computeColumnsPcm(src, sources, frames, format, fftSize, hop, reassign, out) {
    if (src.byteLength !== sources * frames * format.frameBytes) throw Object.assign(new Error('src must hold sources * frames frames'), { code: 'EMSPEC_ERR_INVALID_ARG' });
    return native.batchPcm(this._h, src, format.sampleType, format.channels, format.views, format.mix, sources, fftSize, hop, !!reassign,
      out.db, out.rgba, out.index);
  }

  /** computeColumnsPacked from raw interleaved frames (emspec_batch_pcm_packed); offsets: Float64Array(sources * format.views + 1). */
  computeColumnsPcmPacked(src, sources, frames, format, fftSize, hop, reassign, wire, offsets) {
    if (src.byteLength !== sources * frames * format.frameBytes) throw Object.assign(new Error('src must hold sources * frames frames'), { code: 'EMSPEC_ERR_INVALID_ARG' });
    return native.batchPcmPacked(this._h, src, format.sampleType, format.channels, format.views, format.mix, sources, fftSize, hop,
      !!reassign, wire, offsets);
  }

  /** computeColumnsPacked off the JS thread (libuv pool): resolves with C; offsets are filled when it settles. */
  computeColumnsPackedAsync(pcm, S, L, fftSize, hop, reassign, wire, offsets) {
    return native.batchPackedAsync(this._h, pcm, S, L, fftSize, hop, !!reassign, wire, offsets);
  }

  /**
   * Multi-resolution columns (emspec_batch_multires, DESIGN.md §3.8): a long FFT (opts.lowFftSize, 8192 or 16384) for the
   * rows below the split, the short one (opts.fftSize, 1024 ... 4096) from it up, on one column grid - bass notes a fraction
   * of a short FFT's bin apart separate, transients above the split stay sharp.  opts: {fftSize, lowFftSize, hop,
   * splitHz | splitRow, reassign = true}; splitHz picks the first admissible row whose lower edge is >= splitHz.  out as in
   * computeColumns, S * C * rows cells with C = multiresColumns(L, lowFftSize, fftSize, hop).  Synchronous; returns C.
   */
  computeColumnsMultires(pcm, S, L, opts, out) {
    const split = opts.splitRow !== undefined ? opts.splitRow : this.splitRowForHz(opts.splitHz);
    const reassign = opts.reassign === undefined ? true : !!opts.reassign;
    return native.batchMultires(this._h, pcm, S, L, opts.lowFftSize, opts.fftSize, opts.hop, split, reassign, out.db, out.rgba,
                                out.index);
  }

  /**
   * Multi-band columns (emspec_batch_multiband, DESIGN.md §3.13): two to four FFT sizes, opts.fftSizes[0] > fftSizes[1] > ...
   * (each 1024 ... 16384), fftSizes[k] for the rows from the k-th split up, on the longest FFT's column grid - e.g.
   * [16384, 4096, 1024] with splitHz [250, 2000].  opts: {fftSizes, splitHz | splitRows (one fewer than fftSizes), hop,
   * reassign = true}; each splitHz picks the first admissible row whose lower edge is >= it.  out as in computeColumns,
   * S * C * rows cells with C = multibandColumns(L, fftSizes, hop).  Synchronous; returns C.
   */
  computeColumnsMultiband(pcm, S, L, opts, out) {
    const splits = opts.splitRows !== undefined ? opts.splitRows : Array.from(opts.splitHz, (hz) => this.splitRowForHz(hz));
    const reassign = opts.reassign === undefined ? true : !!opts.reassign;
    return native.batchMultiband(this._h, pcm, S, L, Int32Array.from(opts.fftSizes), Int32Array.from(splits), opts.hop, reassign,
                                 out.db, out.rgba, out.index);
  }

  /** The smallest admissible split row (a multiple of 4 in [64, rows - 64]) whose lower edge is >= hz. */
  splitRowForHz(hz) {
    const e = this.getRowEdges();
    for (let r = 64; r <= this.rows - 64; r += 4) if (e[r] >= Math.fround(hz)) return r;
    const err = new Error(`no admissible split row at or above ${hz} Hz`);
    err.code = 'EMSPEC_ERR_INVALID_ARG';
    throw err;
  }

  /** Same as computeColumns, off the JS thread: resolves with C.  Do not touch the arrays or this
   *  engine until the promise settles (an engine is not thread-safe). */
  computeColumnsAsync(pcm, S, L, fftSize, hop, reassign, out) {
    return native.batchAsync(this._h, pcm, S, L, fftSize, hop, !!reassign, out.db, out.rgba, out.index);
  }

  /** Synchronise the device and throw if a kernel flagged a protocol error since the last check (emspec_device_status). */
  deviceStatus() { native.deviceStatus(this._h); }

  /** Multi-GPU (one node process per GPU): join the gather communicator.  id = commUniqueId() of rank 0, handed over by
   *  the host's own channel (IPC, a file); collective over all `world` rank processes. */
  commInit(id, rank, world) { native.commInit(this._h, id, rank, world); this.commRank = rank; this.commWorld = world; }

  /** This rank's shard of the streams -> finished columns, gathered on `root` over RCCL (packed on the wire).
   *  out.allIndex (root): Uint8Array(world*S*C*rows), rank-major; out.db (optional): this rank's own dB columns.
   *  Returns the bytes this rank put on the wire.  Collective: every rank process calls it. */
  computeColumnsGather(pcm, S, L, fftSize, hop, reassign, root, out) {
    return native.batchGather(this._h, pcm, S, L, fftSize, hop, !!reassign, root, out.allIndex, out.db);
  }

  setColormap(rgba256) { native.setColormap(this._h, rgba256); }

  /** Temporal smoothing (0..0.95) and adaptive brightness / AGC strength (0..1); 0,0 = off. */
  setDisplay(smoothing = 0, agcStrength = 0) { native.setDisplay(this._h, smoothing, agcStrength); }

  /** Install any strictly increasing frequency axis: Float32Array(rows+1) of edges in Hz; null = log axis. */
  setRowEdges(edgesHz) { native.setRowEdges(this._h, edgesHz); }
  /** The axis in use (rows+1 edges in Hz): the inverse map for the shift+hover frequency read-out. */
  getRowEdges() { const e = new Float32Array(this.rows + 1); native.getRowEdges(this._h, e); return e; }
  /** Frequency (Hz) at fractional row y, geometric within the row. */
  rowToHz(y) {
    const e = this.getRowEdges();
    const r = Math.min(this.rows - 1, Math.max(0, Math.floor(y)));
    return e[r] * Math.pow(e[r + 1] / e[r], Math.min(1, Math.max(0, y - r)));
  }
  reset() { native.reset(this._h); }
  destroy() { if (this._h) { native.destroy(this._h); this._h = null; } }
}

/**
 * One [BUILD-DEFINED] law for the reference's "Frequency Scale" (zoom) and "Low-End Boost"
 * sliders (their real laws are undocumented): the axis spans fmin .. fmin*(fmax/fmin)^(1/freqScale)
 * and row r sits at u = (r/rows)^lowEndBoost along the log range, so lowEndBoost > 1 gives the
 * low end more rows.  Returns Float32Array(rows+1) for Engine#setRowEdges.
 */
function warpedEdges(rows, fminHz, fmaxHz, lowEndBoost = 1, freqScale = 1) {
  return native.warpedEdges(rows, fminHz, fmaxHz, lowEndBoost, freqScale);   // one implementation for every host: emspec_warped_edges_hz
}

/** The reference's colour ramp (5-stop gradient measured from its screenshot) with a brightness factor: Uint8Array(1024). */
function makeColormap(brightness = 0.5, stops = undefined) {
  if (stops === undefined) return native.referenceColormap(brightness);   // emspec_make_colormap, shared with the other bindings
  const lut = new Uint8Array(1024);
  const n = stops.length - 1;
  for (let i = 0; i < 256; i++) {
    const v = Math.min(1, (i / 255) * (brightness / 0.5));
    const t = v * n, s = Math.min(n - 1, Math.floor(t)), f = t - s;
    for (let c = 0; c < 3; c++) lut[4 * i + c] = Math.round(stops[s][c] + f * (stops[s + 1][c] - stops[s][c]));
    lut[4 * i + 3] = 255;
  }
  return lut;
}

/** The stereo palette built from makeColormap(brightness) (emspec_make_stereo_colormap): Uint8Array(33 * 1024), [pan][index][4] -
 *  row 16 the colour map itself, rows towards 0 tinted warm (channel a louder), towards 32 cold (channel b louder). */
function makeStereoColormap(brightness = 0.5) { return native.stereoColormap(brightness); }
function stereoMap(map) {
  if (!map) return null;
  return Float32Array.of(map.dbTop, map.dbRange, map.gateDb, map.shiftDb || 0, map.panRangeDb === undefined ? 12 : map.panRangeDb);
}

/** Gradient stop tables for makeColormap().  'reference' is the ramp measured from the reference's
 *  settings screenshot (SURVEY.md §4); the others are plain conveniences, not claims about the
 *  reference's other (undocumented) maps. */
const colormapStops = {
  reference: [[0, 0, 0], [80, 0, 80], [200, 50, 50], [255, 150, 0], [255, 255, 200]],
  grayscale: [[0, 0, 0], [255, 255, 255]],
  ice: [[0, 0, 0], [0, 40, 120], [0, 140, 200], [140, 230, 255], [255, 255, 255]],
  green: [[0, 0, 0], [0, 70, 20], [40, 180, 60], [200, 255, 140], [255, 255, 255]],
};

let defaultEngine = null;
let defaultMulti = null;

/** Drop-in for a renderer that draws S streams: frames = Float32Array(S * fftSize) -> Float32Array(S * rows) of dB
 *  (one launch for all streams).  Lazily creates one engine per stream count. */
function computeSpectrogramColumns(frames, fftSize, hop, reassign = true) {
  const S = frames.length / fftSize;
  if (!defaultMulti || defaultMulti.streams !== S) {
    if (defaultMulti) defaultMulti.destroy();
    defaultMulti = new Engine({ streams: S });
  }
  return defaultMulti.computeSpectrogramColumns(frames, fftSize, hop, reassign);
}

/** Drop-in for the renderer: lazily creates one engine with the default configuration. */
function computeSpectrogramColumn(audioFrame, fftSize, hop, reassign = true) {
  if (!defaultEngine) defaultEngine = new Engine();
  return defaultEngine.computeSpectrogramColumn(audioFrame, fftSize, hop, reassign);
}

/**
 * pcmFormat({type: 's16' | 's24' | 's32' | 'f32', channels, views}) -> the format object the PCM calls take
 * ({type, sampleType, channels, views, mix: Float32Array(views * channels), frameBytes}; emspec_pcm_format).  views: an array of
 * names - 'left', 'right' (channel 0 / 1), 'mid', 'side' (0.5 (ch0 +- ch1)), 'mono' (1 / channels, rounded to float32, on every
 * channel) - and / or arrays of `channels` weights; default ['mono'].  frameBytes is emspec_pcm_frame_bytes: -1 for an invalid
 * format, which the calls then refuse with EMSPEC_ERR_INVALID_ARG naming the field.
 */
const PCM_TYPES = { s16: 1, s24: 2, s32: 3, f32: 4 };
function pcmViewWeights(name, channels) {
  const w = new Array(channels).fill(0);
  if (name === 'mono') return w.fill(Math.fround(1 / channels));
  if (name === 'left') { w[0] = 1; return w; }
  if (channels < 2) throw new Error(`view "${name}" needs at least two channels`);
  if (name === 'right') w[1] = 1;
  else if (name === 'mid') { w[0] = 0.5; w[1] = 0.5; }
  else if (name === 'side') { w[0] = 0.5; w[1] = -0.5; }
  else throw new Error(`unknown view "${name}"`);
  return w;
}
function pcmFormat({ type, channels, views = ['mono'] }) {
  const sampleType = typeof type === 'string' ? (PCM_TYPES[type] || 0) : type | 0;
  const rows = views.map((v) => (typeof v === 'string' ? pcmViewWeights(v, channels) : Array.from(v)));
  const mix = new Float32Array(rows.length * channels);
  rows.forEach((r, v) => {
    if (r.length !== channels) throw new Error('every view needs `channels` weights');
    mix.set(r, v * channels);
  });
  const f = { type, sampleType, channels: channels | 0, views: rows.length, mix };
  f.frameBytes = native.pcmFrameBytes(f.sampleType, f.channels, f.views, f.mix);
  return f;
}

/**
 * The waveform envelope of pcm (Float32Array, S streams of L samples) on the host's own cores (emspec_wave_host: no device, no
 * engine): Float32Array of S x ceil(columns / factor) x (lo, hi), the smallest and the largest sample under each delivered
 * column in the total order of the floats (-0 below +0, NaN skipped; none: +Infinity, -Infinity).
 */
function waveOf(pcm, S, L, fftSize, hop, factor = 1) {
  const C = L >= fftSize && hop >= 1 ? Math.floor((L - fftSize) / hop) + 1 : 0;
  const f = Math.min(65536, Math.max(1, factor | 0));
  const out = new Float32Array(Math.max(0, S) * Math.ceil(C / f) * 2);
  native.waveOf(pcm, S, L, fftSize, hop, factor | 0, out);
  return out;
}

/**
 * Level and cross records (emspec_level: 24 bytes, emspec_cross: 16) as views over one buffer.
 * levelRecords(count): { count, bytes, limbs: BigUint64Array - sq_lo at [3 i], sq_hi at [3 i + 1] -, words: Uint32Array - peak at
 * [6 i + 4], odd at [6 i + 5] };  crossRecords(count): { count, bytes, lo: BigUint64Array - at [2 i] -, hi: BigInt64Array - at
 * [2 i + 1] }.  The sum of squares of record i is limbs[3 i + 1] * 2n ** 32n + limbs[3 i], the sum of products hi * 2n ** 32n + lo.
 */
function levelRecords(count, buf = new ArrayBuffer(Math.max(0, count) * 24)) {   // (buf: e.g. page-locked memory of that size)
  return { count, bytes: new Uint8Array(buf), limbs: new BigUint64Array(buf), words: new Uint32Array(buf) };
}
function crossRecords(count, buf = new ArrayBuffer(Math.max(0, count) * 16)) {
  return { count, bytes: new Uint8Array(buf), lo: new BigUint64Array(buf), hi: new BigInt64Array(buf) };
}
/**
 * The record of several records' samples together (emspec_level_sum / emspec_cross_sum): records [first, first + count) of a
 * levelRecords / crossRecords block summed field by field (the peak: the maximum) -> a block of one record, for levelValues
 * (over count x hop samples) and crossCorrelation.  What a meter that integrates 300 or 400 ms does with the per-hop records of
 * engine.setLiveLevel / setLiveCross.  Throws EMSPEC_ERR_INVALID_ARG for count < 1 or a sum no limb can hold.
 */
function levelSum(level, first = 0, count = level.count - first) {
  const out = levelRecords(1);
  native.levelSum(level.bytes.subarray(24 * first, 24 * (first + Math.max(0, count))), out.bytes);
  return out;
}
function crossSum(cross, first = 0, count = cross.count - first) {
  const out = crossRecords(1);
  native.crossSum(cross.bytes.subarray(16 * first, 16 * (first + Math.max(0, count))), out.bytes);
  return out;
}
function reducedColumnsOf(L, fftSize, hop, factor) {
  const C = L >= fftSize && hop >= 1 ? Math.floor((L - fftSize) / hop) + 1 : 0;
  return Math.ceil(C / Math.min(65536, Math.max(1, factor | 0)));
}
/**
 * The level records of pcm (Float32Array, S streams of L samples) on the host's own cores (emspec_level_host: no device, no
 * engine): levelRecords of S x ceil(columns / factor) - per delivered column the exact sum of squares, the peak and the count of
 * NaN / saturated samples under it, the samples in units of 2^-24.
 */
function levelsOf(pcm, S, L, fftSize, hop, factor = 1) {
  const out = levelRecords(Math.max(0, S) * reducedColumnsOf(L, fftSize, hop, factor));
  native.levelsOf(pcm, S, L, fftSize, hop, factor | 0, out.bytes);
  return out;
}
/** The cross records of pairs of streams (emspec_cross_host): pair p is streams p views + a and p views + b of pcm. */
function crossOf(pcm, pairs, views, a, b, L, fftSize, hop, factor = 1) {
  const out = crossRecords(Math.max(0, pairs) * reducedColumnsOf(L, fftSize, hop, factor));
  native.crossOf(pcm, pairs, views | 0, a | 0, b | 0, L, fftSize, hop, factor | 0, out.bytes);
  return out;
}
/** {rmsDb, peakDb} of level record i over `samples` samples (levelWindow), dB re full scale; -Infinity for silence. */
function levelValues(level, i, samples) {
  const [rmsDb, peakDb] = native.levelValues(level.bytes.subarray(24 * i, 24 * i + 24), samples);
  return { rmsDb, peakDb };
}
/** rho in [-1, 1] of cross record k and its two channels' level records i and j; 0 for silence. */
function crossCorrelation(levelA, i, levelB, j, cross, k) {
  return native.crossCorrelation(levelA.bytes.subarray(24 * i, 24 * i + 24), levelB.bytes.subarray(24 * j, 24 * j + 24),
    cross.bytes.subarray(16 * k, 16 * k + 16));
}

function peaksOf(db, columns, rows, k = 8, minDb = -60) {
  const out = new Float32Array(Math.max(0, columns) * Math.min(32, Math.max(1, k | 0)) * 2);
  native.peaksOf(db, columns, rows, k | 0, +minDb, out);
  return out;
}

const NOTE_NAMES = ['C', 'C#', 'D', 'D#', 'E', 'F', 'F#', 'G', 'G#', 'A', 'A#', 'B'];
function noteOf(hz) {
  const semis = 12 * Math.log2(hz / 440);
  const n = Math.floor(semis + 0.5);
  const midi = 69 + n;
  return { name: NOTE_NAMES[((midi % 12) + 12) % 12], octave: Math.floor(midi / 12) - 1, cents: 100 * (semis - n) };
}

module.exports = {
  pcmFormat,
  Engine,
  createEngine: (config) => new Engine(config),
  computeSpectrogramColumn,
  computeSpectrogramColumns,
  /** ArrayBuffer of page-locked host memory: typed arrays over it move at full PCIe speed. */
  allocPinned: native.allocPinned,
  warpedEdges,
  makeColormap,
  makeStereoColormap,
  colormapStops,
  commUniqueId: native.commUniqueId,
  numColumns: native.numColumns,
  /** Columns per stream a batch call delivers at time reduction f: ceil(columns / f); -1 on invalid arguments. */
  reducedColumns: native.reducedColumns,
  /** Bytes that always hold the wire image of `columns` columns of `rows` rows (emspec_wire_bound). */
  wireBound: native.wireBound,
  /** Expand one wire image (Uint8Array) into out: Uint8Array(columns * rows) on the host's own cores - no device, no engine. */
  unpackWire: native.wireUnpack,
  /** The host twin of computePeaks (emspec_peaks_host; no device, no engine): db = Float32Array(columns * rows), any dB columns
   *  - a live call's, computeColumnsMultires's - -> Float32Array [columns][k][2]. */
  peaksOf,
  waveOf,
  levelRecords,
  crossRecords,
  levelsOf,
  crossOf,
  /** The samples in window g of a stream of L samples (emspec_level_window); 0 where there is none. */
  levelWindow: native.levelWindow,
  levelValues,
  crossCorrelation,
  levelSum,
  crossSum,
  /** hz -> {name, octave, cents}: 12-tone equal temperament around A4 = 440 Hz, the nearest semitone, cents in [-50, 50). */
  noteOf,
  latencyColumns: native.latencyColumns,
  /** Columns of a multi-resolution batch (emspec_multires_columns): multiresColumns(L, lowFftSize, fftSize, hop), -1 for a
   *  shape it does not accept. */
  multiresColumns: native.multiresColumns,
  /** Columns of a multi-band batch (emspec_multiband_columns): multibandColumns(L, fftSizes, hop), -1 for a shape that is not
   *  accepted. */
  multibandColumns: (L, fftSizes, hop) => native.multibandColumns(L, Int32Array.from(fftSizes), hop),
  /** The bands' column shifts (fftSizes[0] - fftSizes[k]) / (2 hop) as an Array, null for a shape that is not accepted
   *  (emspec_multiband_shifts). */
  multibandShifts: (fftSizes, hop) => { const r = native.multibandShifts(Int32Array.from(fftSizes), hop); return r ? Array.from(r) : null; },
  /** 'emspec abi=2 sources=<sha16> arch=gfx950': what the loaded libemspec was built from. */
  buildInfo: native.buildInfo,
};
