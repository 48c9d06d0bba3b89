// The stereo image through the addon (em.makeStereoColormap, engine.setStereoColormap / computeStereo / historyViewStereo), for
// tests/test_gpu_stereo.py:
//   node test_stereo.js <feed.s16> <out.bin> sources frames fftSize hop rows W
// feed: int16 [sources][frames][2], stereo S16.  One EXACT engine of sources * 4 streams (L R M S): the palette of brightness
// 0.7, two computeStereo calls, then a live PCM session fed hop by hop and flushed, the uploaded palette, and two stereo views
// of its history.  Every array is appended to out.bin in order - the Python test makes the same calls through its own binding
// and compares the bytes.  Prints one JSON line.
'use strict';
const fs = require('fs');
const em = require('./index.js');

const [feedPath, outPath] = process.argv.slice(2, 4);
const [sources, frames, fftSize, hop, rows, W] = process.argv.slice(4, 10).map(Number);
const buf = fs.readFileSync(feedPath);
const raw = new Int16Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length));
if (raw.length !== sources * frames * 2) throw new Error(`feed holds ${raw.length} samples, not ${sources * frames * 2}`);

const format = em.pcmFormat({ type: 's16', channels: 2, views: ['left', 'right', 'mid', 'side'] });
const S = sources * format.views;
const engine = em.createEngine({ streams: S, rows, exact: true });
const map = { dbTop: -6, dbRange: 55, gateDb: -58.5, shiftDb: 4.25, panRangeDb: 12 };
const all = ['level', 'index', 'pan', 'rgba'];
const chunks = [];
const keep = (o, names) => { for (const k of names) chunks.push(Buffer.from(o[k].buffer, o[k].byteOffset, o[k].byteLength)); };

const palette = em.makeStereoColormap(0.7);
chunks.push(Buffer.from(palette.buffer, palette.byteOffset, palette.byteLength));
const one = engine.computeStereo(raw, sources, frames, format, fftSize, hop, true, { want: all });
keep(one, all);
keep(engine.computeStereo(raw, sources, frames, format, fftSize, hop, true, { a: 2, b: 3, map }), ['index', 'pan']);

// the live session: one block of `hop` frames per call (the first calls only fill the first frame), then the flushes
engine.setStereoColormap(palette);
engine.setLiveHistory(W);
const block = new Int16Array(sources * hop * 2);
let emitted = 0;
for (let a = 0; a < frames; a += hop) {
  const cnt = Math.min(hop, frames - a);
  const blk = cnt === hop ? block : new Int16Array(sources * cnt * 2);
  for (let s = 0; s < sources; s++) blk.set(raw.subarray((s * frames + a) * 2, (s * frames + a + cnt) * 2), s * cnt * 2);
  emitted += engine.pushSamplesPcm(blk, format, { fftSize, hop }).counts[0];
}
const D = em.latencyColumns(fftSize, hop, true);
for (let i = 0; i < D; i++) { engine.flushColumns(); emitted++; }
const first = emitted - W;
keep(engine.historyViewStereo({ views: 4, a: 0, b: 1, firstColumn: first, groups: W, want: all }), all);
keep(engine.historyViewStereo({ stream0: 4, pairs: 1, views: 4, a: 2, b: 3, firstColumn: first + 1, factor: 2, groups: 2, map, want: all }), all);
fs.writeFileSync(outPath, Buffer.concat(chunks));

// refusals leave the engine usable
let code = 'none';
try { engine.historyViewStereo({ views: 4, a: 1, b: 1, firstColumn: first, groups: 1 }); } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`a pair of one channel gave ${code}`);
try { engine.computeStereo(raw, sources, frames, format, fftSize, hop, true, { a: 0, b: 4 }); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`a channel outside the views gave ${code}`);
if (engine.historyViewStereo({ views: 4, firstColumn: first, groups: 1 }).pan.length !== sources * rows) throw new Error('a view after the refusals');
engine.destroy();
console.log(JSON.stringify({ ok: true, S, columns: one.columns, emitted, first }));
