// The live multi-band session through the addon (engine.pushSamplesMultiband, computeSpectrogramColumnsMultiband, flushColumns),
// for tests/test_gpu_live_multiband.py: writes the input and the emitted dB / RGBA columns to the directory in argv[2]; the test
// feeds the same blocks through the ctypes binding and compares the bytes.  EXACT engine: the bytes are reproducible.
'use strict';
const fs = require('fs');
const path = require('path');
const em = require('./index.js');

const outDir = process.argv[2];
const S = 4, fftSizes = [4096, 2048, 1024], hop = 256, splitHz = [250, 2000], block = 1000;
const L = fftSizes[0] + hop * 59;
const pcm = new Float32Array(S * L);
for (let s = 0; s < S; s++)
  for (let i = 0; i < L; i++)
    pcm[s * L + i] = 0.3 * Math.sin(2 * Math.PI * (41.2 + 7.8 * s) * i / 48000) + 0.2 * Math.sin(2 * Math.PI * 1234.5 * i / 48000) +
                     (i % 12000 === 0 ? 0.5 : 0);

const engine = em.createEngine({ exact: true, streams: S });
const R = engine.rows, J = em.multibandColumns(L, Int32Array.from(fftSizes), hop);
const opts = { fftSizes, hop, splitHz, wantRgba: true };
const db = new Float32Array(S * J * R), rgba = new Uint8Array(4 * S * J * R);
const next = new Array(S).fill(0);
for (let a = 0; a < L; a += block) {
  const cnt = Math.min(block, L - a);
  const blk = engine.sampleBlock(cnt);
  for (let s = 0; s < S; s++) blk.set(pcm.subarray(s * L + a, s * L + a + cnt), s * cnt);
  const r = engine.pushSamplesMultiband(blk, opts);
  for (let s = 0; s < S; s++)
    for (let i = 0; i < r.counts[s]; i++) {
      if (r.first[s] + i !== next[s]) throw new Error(`stream ${s}: column ${r.first[s] + i}, expected ${next[s]}`);
      const from = (s * r.maxColumns + i) * R, to = (s * J + next[s]++) * R;
      db.set(r.db.subarray(from, from + R), to);
      rgba.set(r.rgba.subarray(4 * from, 4 * (from + R)), 4 * to);
    }
}
// a single-resolution live call, or the per-frame form, on the multi-band session of sample blocks is a state error
for (const bad of [() => engine.pushSamplesMulti(engine.sampleBlock(hop), fftSizes[0], hop, true),
                   () => engine.computeSpectrogramColumnsMultiband(new Float32Array(S * fftSizes[0]), opts)]) {
  let threw = false;
  try { bad(); } catch (e) { threw = e.code === 'EMSPEC_ERR_STATE'; }
  if (!threw) throw new Error('a call of another kind on the multi-band session was not refused');
}
// a shape the band rule rejects names the rule
let named = false;
try { engine.pushSamplesMultiband(engine.sampleBlock(hop), { fftSizes: [2048, 4096], hop, splitRows: [512] }); } catch (e) {
  named = e.code === 'EMSPEC_ERR_INVALID_ARG' && /strictly decreasing/.test(e.message);
}
if (!named) throw new Error('an increasing ladder was not refused with the rule');
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
// the per-frame form after reset(): the first D calls emit the empty column, then column 0 equals the pushed session's
engine.reset();
const D = em.latencyColumns(fftSizes[0], hop, true);
let frame0Equal = true;
for (let j = 0; j <= D; j++) {
  const frames = new Float32Array(S * fftSizes[0]);
  for (let s = 0; s < S; s++) frames.set(pcm.subarray(s * L + j * hop, s * L + j * hop + fftSizes[0]), s * fftSizes[0]);
  const col = engine.computeSpectrogramColumnsMultiband(frames, opts);
  for (let s = 0; s < S; s++) {
    if (engine.columnIndex[s] !== (j < D ? -1 : 0)) throw new Error(`per-frame: stream ${s} call ${j} column ${engine.columnIndex[s]}`);
    if (j === D) for (let r = 0; r < R; r++) if (col[s * R + r] !== db[s * J * R + r]) frame0Equal = false;
  }
}
if (!frame0Equal) throw new Error('the per-frame form\'s column 0 differs from the block form\'s');
const splitRows = splitHz.map((hz) => engine.splitRowForHz(hz));
engine.destroy();

fs.writeFileSync(path.join(outDir, 'pcm.f32'), Buffer.from(pcm.buffer));
fs.writeFileSync(path.join(outDir, 'db.f32'), Buffer.from(db.buffer));
fs.writeFileSync(path.join(outDir, 'rgba.u8'), Buffer.from(rgba.buffer));
console.log(JSON.stringify({ S, L, fftSizes, hop, splitHz, splitRows, block, columns: J, rows: R }));
