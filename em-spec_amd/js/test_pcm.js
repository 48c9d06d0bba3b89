// The PCM front end through the addon (pcmFormat, engine.computeColumnsPcm, engine.computeColumnsPcmPacked,
// engine.pushSamplesPcm, flushColumns), for tests/test_gpu_pcm.py: writes the raw input and the bytes it got to the directory in
// argv[2]; the test makes the same calls through the ctypes binding and compares.  EXACT engine: the bytes are reproducible.
'use strict';
const fs = require('fs');
const path = require('path');
const em = require('./index.js');

const outDir = process.argv[2];
const sources = 2, fftSize = 4096, hop = 256, block = 1000;
const frames = fftSize + hop * 59 + 3;
const format = em.pcmFormat({ type: 's16', channels: 2, views: ['left', 'right', 'mid', 'side'] });
if (format.frameBytes !== 4) throw new Error(`frameBytes ${format.frameBytes}`);
const S = sources * format.views;
const src = new Int16Array(sources * frames * 2);
for (let s = 0; s < sources; s++)
  for (let i = 0; i < frames; i++) {
    src[(s * frames + i) * 2] = Math.round(9000 * Math.sin(2 * Math.PI * (110 + 60 * s) * i / 48000) + 3000 * Math.sin(2 * Math.PI * 2345.6 * i / 48000));
    src[(s * frames + i) * 2 + 1] = Math.round(7000 * Math.sin(2 * Math.PI * (331 + 40 * s) * i / 48000 + 1) + (i % 9000 === 0 ? 12000 : 0));
  }

const engine = em.createEngine({ exact: true, streams: S });
const R = engine.rows, J = em.numColumns(frames, fftSize, hop);
// batch
const bdb = new Float32Array(S * J * R), bidx = new Uint8Array(S * J * R);
if (engine.computeColumnsPcm(src, sources, frames, format, fftSize, hop, true, { db: bdb, index: bidx }) !== J) throw new Error('columns');
// packed batch: every image expands to the batch's index columns
const wire = new Uint8Array(S * em.wireBound(J, R)), offsets = new Float64Array(S + 1), img = new Uint8Array(J * R);
engine.computeColumnsPcmPacked(src, sources, frames, format, fftSize, hop, true, wire, offsets);
for (let s = 0; s < S; s++) {
  if (offsets[s] % 16) throw new Error('offset alignment');
  em.unpackWire(wire.subarray(offsets[s], offsets[s + 1]), J, R, img);
  for (let i = 0; i < J * R; i++) if (img[i] !== bidx[s * J * R + i]) throw new Error(`packed image of stream ${s} differs at ${i}`);
}
// a typed array whose element type contradicts format.type
for (const bad of [new Float32Array(src.length), new Uint8Array(src.buffer), new Int32Array(src.length)]) {
  let code;
  try { engine.computeColumnsPcm(bad, sources, bad.byteLength / (sources * 4), format, fftSize, hop, true, { db: bdb }); } catch (e) { code = e.code; }
  if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`a ${bad.constructor.name} for an s16 format gave ${code}`);
}
// live, in blocks
const db = new Float32Array(S * J * R), rgba = new Uint8Array(4 * S * J * R);
const next = new Array(S).fill(0);
for (let a = 0; a < frames; a += block) {
  const cnt = Math.min(block, frames - a);
  const blk = new Int16Array(sources * cnt * 2);
  for (let s = 0; s < sources; s++) blk.set(src.subarray((s * frames + a) * 2, (s * frames + a + cnt) * 2), s * cnt * 2);
  const r = engine.pushSamplesPcm(blk, format, { fftSize, hop, wantRgba: true });
  for (let s = 0; s < S; s++)
    for (let i = 0; i < r.counts[s]; i++) {
      if (r.first[s] + i !== next[s]) throw new Error(`stream ${s}: column ${r.first[s] + i}, expected ${next[s]}`);
      const from = (s * r.maxColumns + i) * R, to = (s * J + next[s]++) * R;
      db.set(r.db.subarray(from, from + R), to);
      rgba.set(r.rgba.subarray(4 * from, 4 * (from + R)), 4 * to);
    }
}
// a float live call on the PCM session is a state error
let threw = false;
try { engine.pushSamplesMulti(new Float32Array(S * hop), fftSize, hop, true); } catch (e) { threw = e.code === 'EMSPEC_ERR_STATE'; }
if (!threw) throw new Error('a float call on a PCM session was not refused');
for (;;) {
  try { engine.flushColumns(true); } catch (e) { if (e.code === 'EMSPEC_ERR_STATE') break; throw e; }
  for (let s = 0; s < S; s++) {
    if (engine.columnIndex[s] !== next[s]) throw new Error(`flush: stream ${s} column ${engine.columnIndex[s]}, expected ${next[s]}`);
    const to = (s * J + next[s]++) * R;
    db.set(engine.columnsDb.subarray(s * R, (s + 1) * R), to);
    rgba.set(engine.columnsRgba.subarray(4 * s * R, 4 * (s + 1) * R), 4 * to);
  }
}
for (let s = 0; s < S; s++) if (next[s] !== J) throw new Error(`stream ${s} emitted ${next[s]} of ${J} columns`);
engine.destroy();

fs.writeFileSync(path.join(outDir, 'src.i16'), Buffer.from(src.buffer));
fs.writeFileSync(path.join(outDir, 'batch_db.f32'), Buffer.from(bdb.buffer));
fs.writeFileSync(path.join(outDir, 'batch_index.u8'), Buffer.from(bidx.buffer));
fs.writeFileSync(path.join(outDir, 'db.f32'), Buffer.from(db.buffer));
fs.writeFileSync(path.join(outDir, 'rgba.u8'), Buffer.from(rgba.buffer));
console.log(JSON.stringify({ sources, views: format.views, frames, fftSize, hop, block, columns: J, rows: R, mix: Array.from(format.mix) }));
