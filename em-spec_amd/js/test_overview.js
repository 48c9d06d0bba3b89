// The time reduction through the addon (createEngine({timeReduce}), engine.setTimeReduce, em.reducedColumns), for
// tests/test_gpu_overview.py: writes the input and the reduced dB / palette-index bytes of computeColumns, computeColumnsPacked
// (expanded with unpackWire) and computeColumnsMultires to the directory in argv[2]; the test runs the same input through the
// ctypes binding and compares the bytes.  EXACT engine: the bytes are reproducible.
'use strict';
const fs = require('fs');
const path = require('path');
const em = require('./index.js');

const outDir = process.argv[2];
const S = 3, L = 1 << 17, lowFftSize = 16384, fftSize = 4096, hop = 256, splitHz = 250, timeReduce = 6;
const pcm = new Float32Array(S * L);
for (let s = 0; s < S; s++)
  for (let i = 0; i < L; i++)
    pcm[s * L + i] = 0.3 * Math.sin(2 * Math.PI * (41.2 + 7.8 * s) * i / 48000) + 0.2 * Math.sin(2 * Math.PI * 1234.5 * i / 48000) +
                     (i % 12000 === 0 ? 0.5 : 0);

if (em.reducedColumns(100, 7) !== 15 || em.reducedColumns(98, 7) !== 14 || em.reducedColumns(5, 65536) !== 1) throw new Error('reducedColumns');
if (em.reducedColumns(100, 0) !== -1 || em.reducedColumns(100, 65537) !== -1 || em.reducedColumns(-1, 2) !== -1) throw new Error('reducedColumns accepted bad arguments');

const engine = em.createEngine({ exact: true, timeReduce });
if (engine.timeReduce !== timeReduce) throw new Error(`timeReduce ${engine.timeReduce}`);
const R = engine.rows;
const Cfull = em.numColumns(L, fftSize, hop), C = em.reducedColumns(Cfull, timeReduce);

// computeColumns: arrays of the reduced size; the full-rate size is refused before anything runs
const out = { db: new Float32Array(S * C * R), index: new Uint8Array(S * C * R) };
const got = engine.computeColumns(pcm, S, L, fftSize, hop, true, out);
if (got !== C) throw new Error(`computeColumns returned ${got}, expected ${C}`);
let threw = false;
try { engine.computeColumns(pcm, S, L, fftSize, hop, true, { index: new Uint8Array(S * Cfull * R) }); } catch (e) { threw = e.code === 'EMSPEC_ERR_INVALID_ARG'; }
if (!threw) throw new Error('full-rate output arrays were not refused');

// computeColumnsPacked: images of the reduced columns
const wire = new Uint8Array(S * em.wireBound(C, R)), offsets = new Float64Array(S + 1);
if (engine.computeColumnsPacked(pcm, S, L, fftSize, hop, true, wire, offsets) !== C) throw new Error('computeColumnsPacked column count');
const packed = new Uint8Array(S * C * R);
for (let s = 0; s < S; s++) em.unpackWire(wire.subarray(offsets[s], offsets[s + 1]), C, R, packed.subarray(s * C * R, (s + 1) * C * R));

// computeColumnsMultires
const Cm = em.reducedColumns(em.multiresColumns(L, lowFftSize, fftSize, hop), timeReduce);
const multi = { index: new Uint8Array(S * Cm * R) };
if (engine.computeColumnsMultires(pcm, S, L, { fftSize, lowFftSize, hop, splitHz }, multi) !== Cm) throw new Error('computeColumnsMultires column count');

// the setter: refusals carry the library's code; the live call refuses while the factor is above 1; factor 1 restores it
for (const bad of [0, -1, 65537]) {
  threw = false;
  try { engine.setTimeReduce(bad); } catch (e) { threw = e.code === 'EMSPEC_ERR_INVALID_ARG'; }
  if (!threw || engine.timeReduce !== timeReduce) throw new Error(`setTimeReduce(${bad}) was not refused`);
}
threw = false;
try { engine.computeSpectrogramColumn(pcm.subarray(0, fftSize), fftSize, hop, true); } catch (e) {
  threw = e.code === 'EMSPEC_ERR_STATE' && /emspec_set_time_reduce/.test(e.message);
}
if (!threw) throw new Error('the live call was not refused');
engine.setTimeReduce(1);
const fullIdx = { index: new Uint8Array(S * Cfull * R) };
if (engine.computeColumns(pcm, S, L, fftSize, hop, true, fullIdx) !== Cfull) throw new Error('factor 1 column count');
// the reduced index is the maximum over each group of the full-rate one
for (let s = 0; s < S; s++)
  for (let g = 0; g < C; g++)
    for (let r = 0; r < R; r += 37) {
      let m = 0;
      for (let c = g * timeReduce; c < Math.min((g + 1) * timeReduce, Cfull); c++) m = Math.max(m, fullIdx.index[(s * Cfull + c) * R + r]);
      if (m !== out.index[(s * C + g) * R + r]) throw new Error(`reduced index differs at ${s},${g},${r}`);
    }
engine.destroy();

fs.writeFileSync(path.join(outDir, 'pcm.f32'), Buffer.from(pcm.buffer));
fs.writeFileSync(path.join(outDir, 'db.f32'), Buffer.from(out.db.buffer));
fs.writeFileSync(path.join(outDir, 'index.u8'), Buffer.from(out.index.buffer));
fs.writeFileSync(path.join(outDir, 'packed_index.u8'), Buffer.from(packed.buffer));
fs.writeFileSync(path.join(outDir, 'multires_index.u8'), Buffer.from(multi.index.buffer));
console.log(JSON.stringify({ S, L, lowFftSize, fftSize, hop, splitHz, timeReduce, columns: C, multiresColumns: Cm, rows: R }));
