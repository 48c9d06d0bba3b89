// The live multi-resolution session through the addon (engine.pushSamplesMultires, flushColumns), for
// tests/test_gpu_live_multires.py: writes the input and the emitted dB / RGBA columns to the directory in argv[2]; the test
// feeds the same blocks through the ctypes binding and compares the bytes.  EXACT engine: the bytes are reproducible.
'use strict';
const fs = require('fs');
const path = require('path');
const em = require('./index.js');

const outDir = process.argv[2];
const S = 4, lowFftSize = 16384, fftSize = 4096, hop = 256, splitHz = 250, block = 1000;
const L = lowFftSize + hop * 59;
const pcm = new Float32Array(S * L);
for (let s = 0; s < S; s++)
  for (let i = 0; i < L; i++)
    pcm[s * L + i] = 0.3 * Math.sin(2 * Math.PI * (41.2 + 7.8 * s) * i / 48000) + 0.2 * Math.sin(2 * Math.PI * 1234.5 * i / 48000) +
                     (i % 12000 === 0 ? 0.5 : 0);

const engine = em.createEngine({ exact: true, streams: S });
const R = engine.rows, J = em.multiresColumns(L, lowFftSize, fftSize, hop);
const opts = { fftSize, lowFftSize, hop, splitHz, wantRgba: true };
const db = new Float32Array(S * J * R), rgba = new Uint8Array(4 * S * J * R);
const next = new Array(S).fill(0);
for (let a = 0; a < L; a += block) {
  const cnt = Math.min(block, L - a);
  const blk = engine.sampleBlock(cnt);
  for (let s = 0; s < S; s++) blk.set(pcm.subarray(s * L + a, s * L + a + cnt), s * cnt);
  const r = engine.pushSamplesMultires(blk, opts);
  for (let s = 0; s < S; s++)
    for (let i = 0; i < r.counts[s]; i++) {
      if (r.first[s] + i !== next[s]) throw new Error(`stream ${s}: column ${r.first[s] + i}, expected ${next[s]}`);
      const from = (s * r.maxColumns + i) * R, to = (s * J + next[s]++) * R;
      db.set(r.db.subarray(from, from + R), to);
      rgba.set(r.rgba.subarray(4 * from, 4 * (from + R)), 4 * to);
    }
}
// a single-resolution live call on the multi-resolution session is a state error
let threw = false;
try { engine.pushSamplesMulti(engine.sampleBlock(hop), fftSize, hop, true); } catch (e) { threw = e.code === 'EMSPEC_ERR_STATE'; }
if (!threw) throw new Error('a single-resolution call on a multi-resolution session was not refused');
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
const splitRow = engine.splitRowForHz(splitHz);
engine.destroy();

fs.writeFileSync(path.join(outDir, 'pcm.f32'), Buffer.from(pcm.buffer));
fs.writeFileSync(path.join(outDir, 'db.f32'), Buffer.from(db.buffer));
fs.writeFileSync(path.join(outDir, 'rgba.u8'), Buffer.from(rgba.buffer));
console.log(JSON.stringify({ S, L, lowFftSize, fftSize, hop, splitHz, splitRow, block, columns: J, rows: R }));
