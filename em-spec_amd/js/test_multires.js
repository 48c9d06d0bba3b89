// Multi-resolution columns through the addon (engine.computeColumnsMultires, em.multiresColumns), for
// tests/test_gpu_multires.py: writes the input and the palette-index bytes to the directory in argv[2]; the test runs the
// same input through the ctypes binding and compares the bytes.  EXACT engine: the bytes are reproducible.
'use strict';
const fs = require('fs');
const path = require('path');
const em = require('./index.js');

const outDir = process.argv[2];
const S = 2, L = 1 << 17, lowFftSize = 16384, fftSize = 4096, hop = 256, splitHz = 250;
const pcm = new Float32Array(S * L);
for (let s = 0; s < S; s++)
  for (let i = 0; i < L; i++)
    pcm[s * L + i] = 0.3 * Math.sin(2 * Math.PI * (41.2 + 7.8 * s) * i / 48000) + 0.2 * Math.sin(2 * Math.PI * 1234.5 * i / 48000) +
                     (i % 12000 === 0 ? 0.5 : 0);

const C = em.multiresColumns(L, lowFftSize, fftSize, hop);
if (C !== em.numColumns(L, lowFftSize, hop)) throw new Error(`multiresColumns ${C}`);
if (em.multiresColumns(L, 16384, 2048, 1000) !== -1) throw new Error('multiresColumns accepted a non-integer shift');

const engine = em.createEngine({ exact: true });
const out = { index: new Uint8Array(S * C * engine.rows) };
const got = engine.computeColumnsMultires(pcm, S, L, { fftSize, lowFftSize, hop, splitHz }, out);
if (got !== C) throw new Error(`computeColumnsMultires returned ${got}, expected ${C}`);
const splitRow = engine.splitRowForHz(splitHz);
// splitRow given directly: the same bytes
const again = { index: new Uint8Array(S * C * engine.rows) };
engine.computeColumnsMultires(pcm, S, L, { fftSize, lowFftSize, hop, splitRow }, again);
if (Buffer.compare(Buffer.from(out.index), Buffer.from(again.index)) !== 0) throw new Error('splitHz and splitRow differ');
// a rejected shape throws with the library's code and message
let threw = false;
try { engine.computeColumnsMultires(pcm, S, L, { fftSize: 2048, lowFftSize, hop: 1000, splitRow }, again); } catch (e) {
  threw = e.code === 'EMSPEC_ERR_INVALID_ARG' && /integer/.test(e.message);
}
if (!threw) throw new Error('a non-integer shift was not rejected');
engine.destroy();

fs.writeFileSync(path.join(outDir, 'pcm.f32'), Buffer.from(pcm.buffer));
fs.writeFileSync(path.join(outDir, 'index.u8'), Buffer.from(out.index.buffer));
console.log(JSON.stringify({ S, L, lowFftSize, fftSize, hop, splitHz, splitRow, columns: C, rows: engine.rows }));
