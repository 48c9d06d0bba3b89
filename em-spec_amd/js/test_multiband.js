// Multi-band columns through the addon (engine.computeColumnsMultiband, em.multibandColumns, em.multibandShifts), for
// tests/test_gpu_multiband.py: writes the input and the palette-index bytes to the directory in argv[2]; the test runs the
// same input through the ctypes binding and compares the bytes.  EXACT engine: the bytes are reproducible.
'use strict';
const fs = require('fs');
const path = require('path');
const em = require('./index.js');

const outDir = process.argv[2];
const S = 2, L = 1 << 17, fftSizes = [16384, 4096, 1024], hop = 256, splitHz = [250, 2000];
const pcm = new Float32Array(S * L);
for (let s = 0; s < S; s++)
  for (let i = 0; i < L; i++)
    pcm[s * L + i] = 0.3 * Math.sin(2 * Math.PI * (41.2 + 7.8 * s) * i / 48000) + 0.2 * Math.sin(2 * Math.PI * 1234.5 * i / 48000) +
                     0.1 * Math.sin(2 * Math.PI * 8000 * i / 48000) + (i % 12000 === 0 ? 0.5 : 0);

const C = em.multibandColumns(L, fftSizes, hop);
if (C !== em.numColumns(L, fftSizes[0], hop)) throw new Error(`multibandColumns ${C}`);
if (em.multibandColumns(L, [16384, 4096, 2048], 1000) !== -1) throw new Error('multibandColumns accepted a non-integer shift');
const shifts = em.multibandShifts(fftSizes, hop);
if (JSON.stringify(shifts) !== '[0,24,30]') throw new Error(`multibandShifts ${JSON.stringify(shifts)}`);
if (em.multibandShifts([16384, 4096, 512], hop) !== null) throw new Error('multibandShifts accepted a size of 512');
// two bands: the columns of the two-band function
if (em.multibandColumns(L, [16384, 4096], hop) !== em.multiresColumns(L, 16384, 4096, hop)) throw new Error('two bands: columns differ');

const engine = em.createEngine({ exact: true });
const out = { index: new Uint8Array(S * C * engine.rows) };
const got = engine.computeColumnsMultiband(pcm, S, L, { fftSizes, hop, splitHz }, out);
if (got !== C) throw new Error(`computeColumnsMultiband returned ${got}, expected ${C}`);
const splitRows = splitHz.map((hz) => engine.splitRowForHz(hz));
// splitRows given directly: the same bytes
const again = { index: new Uint8Array(S * C * engine.rows) };
engine.computeColumnsMultiband(pcm, S, L, { fftSizes, hop, splitRows }, again);
if (Buffer.compare(Buffer.from(out.index), Buffer.from(again.index)) !== 0) throw new Error('splitHz and splitRows differ');
// two bands: the bytes of computeColumnsMultires
const two = { index: new Uint8Array(S * C * engine.rows) }, twin = { index: new Uint8Array(S * C * engine.rows) };
engine.computeColumnsMultiband(pcm, S, L, { fftSizes: [16384, 4096], hop, splitRows: [splitRows[0]] }, two);
engine.computeColumnsMultires(pcm, S, L, { fftSize: 4096, lowFftSize: 16384, hop, splitRow: splitRows[0] }, twin);
if (Buffer.compare(Buffer.from(two.index), Buffer.from(twin.index)) !== 0) throw new Error('two bands differ from computeColumnsMultires');
// rejected shapes throw with the library's code and message
const rejected = (opts, rule) => {
  try { engine.computeColumnsMultiband(pcm, S, L, opts, again); } catch (e) { return e.code === 'EMSPEC_ERR_INVALID_ARG' && rule.test(e.message); }
  return false;
};
if (!rejected({ fftSizes: [16384, 4096, 2048], hop: 1000, splitRows }, /integer/)) throw new Error('a non-integer shift was not rejected');
if (!rejected({ fftSizes, hop, splitRows: [368, 428] }, /64 rows/)) throw new Error('a band of 60 rows was not rejected');
if (!rejected({ fftSizes: [16384], hop, splitRows: [] }, /bands/)) throw new Error('one band was not rejected');
engine.destroy();

fs.writeFileSync(path.join(outDir, 'pcm.f32'), Buffer.from(pcm.buffer));
fs.writeFileSync(path.join(outDir, 'index.u8'), Buffer.from(out.index.buffer));
console.log(JSON.stringify({ S, L, fftSizes, hop, splitHz, splitRows, shifts, columns: C, rows: engine.rows }));
