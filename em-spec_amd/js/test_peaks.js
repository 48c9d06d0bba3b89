// The spectral peaks through the addon (engine.computePeaks, em.peaksOf, engine.positionToHz, em.noteOf), for
// tests/test_gpu_peaks.py: writes the input, computePeaks' lists and peaksOf's lists of computeColumns' dB to the directory in
// argv[2]; the test runs the same input through the ctypes binding and compares the bytes.  EXACT engine: the bytes are
// reproducible.
'use strict';
const fs = require('fs');
const path = require('path');
const em = require('./index.js');

const outDir = process.argv[2];
const S = 3, L = 1 << 16, fftSize = 4096, hop = 256, k = 6, minDb = -55;
const pcm = new Float32Array(S * L);
for (let s = 0; s < S; s++)
  for (let i = 0; i < L; i++)
    pcm[s * L + i] = 0.3 * Math.sin(2 * Math.PI * (220 + 110 * s) * i / 48000) + 0.2 * Math.sin(2 * Math.PI * 1234.5 * i / 48000) +
                     0.05 * Math.sin(2 * Math.PI * 5000 * i / 48000) + (i % 12000 === 0 ? 0.5 : 0);

const engine = em.createEngine({ exact: true });
const R = engine.rows, C = em.numColumns(L, fftSize, hop);
const peaks = engine.computePeaks(pcm, S, fftSize, hop, true, { k, minDb });
if (!(peaks instanceof Float32Array) || peaks.length !== S * C * k * 2) throw new Error(`computePeaks returned ${peaks.length} floats`);
if (engine.computePeaks(pcm, S, fftSize, hop, true).length !== S * C * 8 * 2) throw new Error('the default k is not 8');

const out = { db: new Float32Array(S * C * R) };
engine.computeColumns(pcm, S, L, fftSize, hop, true, out);
const peaksOf = em.peaksOf(out.db, S * C, R, k, minDb);
if (peaksOf.length !== peaks.length) throw new Error('peaksOf length');

// refusals carry the library's code and message
const refused = (f, code, re) => {
  try { f(); } catch (e) { if (e.code === code && re.test(e.message)) return; throw new Error(`wrong refusal: ${e.code} ${e.message}`); }
  throw new Error(`not refused: ${f}`);
};
refused(() => engine.computePeaks(pcm, S, fftSize, hop, true, { k: 33 }), 'EMSPEC_ERR_INVALID_ARG', /k must be/);
refused(() => engine.computePeaks(pcm, S, fftSize, hop, true, { minDb: NaN }), 'EMSPEC_ERR_INVALID_ARG', /NaN/);
refused(() => em.peaksOf(out.db, S * C, R, 0, minDb), 'EMSPEC_ERR_INVALID_ARG', /k must be/);
refused(() => engine.positionToHz(R + 1), 'EMSPEC_ERR_INVALID_ARG', /pos must be/);
engine.setTimeReduce(2);
refused(() => engine.computePeaks(pcm, S, fftSize, hop, true, { k, minDb }), 'EMSPEC_ERR_STATE', /time reduction/);
engine.setTimeReduce(1);

// positionToHz: edges at integer positions, and the hover read-out of the loudest peak of a late column
const edges = engine.getRowEdges();
if (Math.abs(engine.positionToHz(0) / edges[0] - 1) > 1e-12 || Math.abs(engine.positionToHz(R) / edges[R] - 1) > 1e-12) throw new Error('positionToHz at the ends');
const positions = [0, 0.5, 17.25, R - 0.5, R, peaks[((0 * C + 203) * k) * 2]];
const hz = positions.map((p) => engine.positionToHz(p));
const top = em.noteOf(hz[hz.length - 1]);
if (top.name !== 'A' || top.octave !== 3) throw new Error(`the 220 Hz tone reads ${JSON.stringify(top)}`);
const notes = [440, 261.6256, 27.5, 466.1638].map((f) => Object.assign({ hz: f }, em.noteOf(f)));
if (notes[3].name !== 'A#' || notes[3].octave !== 4 || !(notes[3].cents >= -50 && notes[3].cents < 50)) throw new Error('noteOf(466.16)');
engine.destroy();

fs.writeFileSync(path.join(outDir, 'pcm.f32'), Buffer.from(pcm.buffer));
fs.writeFileSync(path.join(outDir, 'peaks.f32'), Buffer.from(peaks.buffer));
fs.writeFileSync(path.join(outDir, 'peaks_of.f32'), Buffer.from(peaksOf.buffer));
console.log(JSON.stringify({ S, L, fftSize, hop, k, minDb, columns: C, rows: R, positions, hz, notes }));
