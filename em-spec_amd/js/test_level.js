// The level meters through the addon (engine.setLevelOut / setCrossOut with engine.computeColumnsPcmPacked, levelsOf, crossOf,
// levelValues, crossCorrelation), for tests/test_gpu_level_node.py: writes the raw input and the bytes it got to the directory in
// argv[2]; the test computes the same records with the Python reference and compares.
'use strict';
const fs = require('fs');
const path = require('path');
const em = require('./index.js');

const outDir = process.argv[2];
const sources = 2, fftSize = 4096, hop = 256, factor = 3;
const frames = fftSize + hop * 29 + 3;
const format = em.pcmFormat({ type: 's16', channels: 2, views: ['left', 'right', 'mid', 'side'] });
const S = sources * format.views;
const src = new Int16Array(sources * frames * 2);
for (let i = 0; i < frames; i++) {
  src[i * 2] = Math.round(9000 * Math.sin(2 * Math.PI * 110 * i / 48000) + 3000 * Math.sin(2 * Math.PI * 2345.6 * i / 48000));
  src[i * 2 + 1] = Math.round(7000 * Math.sin(2 * Math.PI * 331 * i / 48000 + 1) + (i % 9000 === 0 ? 12000 : 0));
  src[(frames + i) * 2] = Math.round(8000 * Math.sin(2 * Math.PI * 170 * i / 48000));   // source 1: right = -left
  src[(frames + i) * 2 + 1] = -src[(frames + i) * 2];
}

const engine = em.createEngine({ exact: true, streams: S, timeReduce: factor });
const R = engine.rows, J = em.numColumns(frames, fftSize, hop), Jr = Math.ceil(J / factor);
const wire = new Uint8Array(S * em.wireBound(Jr, R)), offsets = new Float64Array(S + 1);
const level = em.levelRecords(S * Jr + 1), cross = em.crossRecords(sources * Jr + 1);   // (one record more than needed: it stays)
level.bytes.fill(0xA5); cross.bytes.fill(0xA5);
engine.setLevelOut(level);
engine.setCrossOut(0, 1, cross);
engine.computeColumnsPcmPacked(src, sources, frames, format, fftSize, hop, true, wire, offsets);
for (let i = 0; i < 24; i++) if (level.bytes[S * Jr * 24 + i] !== 0xA5) throw new Error('level records were written past streams x columns');
for (let i = 0; i < 16; i++) if (cross.bytes[sources * Jr * 16 + i] !== 0xA5) throw new Error('cross records were written past sources x columns');
// the helpers: source 1's channels are inverted copies
const rho = em.crossCorrelation(level, 4 * Jr, level, 5 * Jr, cross, Jr);
if (rho !== -1) throw new Error(`an inverted channel correlates ${rho}`);
const samples = em.levelWindow(frames, fftSize, hop, factor, 0);
if (samples !== factor * hop) throw new Error(`window 0 holds ${samples} samples`);
const values = em.levelValues(level, 4 * Jr, samples);
const sum = Number(level.limbs[3 * 4 * Jr + 1]) * 2 ** 32 + Number(level.limbs[3 * 4 * Jr]);
if (Math.abs(values.rmsDb - (10 * Math.log10(sum / samples) - 20 * Math.log10(2 ** 24))) > 1e-9) throw new Error(`rmsDb ${values.rmsDb}`);
if (!(values.peakDb > values.rmsDb && values.peakDb < 0)) throw new Error(`peakDb ${values.peakDb}`);
// one record short, views outside the format, a float-stream call while cross records are set: refused, the engine stays usable
let code;
engine.setLevelOut(em.levelRecords(S * Jr - 1));
try { engine.computeColumnsPcmPacked(src, sources, frames, format, fftSize, hop, true, wire, offsets); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`level records one short gave ${code}`);
engine.setLevelOut(null);
engine.setCrossOut(0, 4, cross);
try { engine.computeColumnsPcmPacked(src, sources, frames, format, fftSize, hop, true, wire, offsets); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`a view outside the format gave ${code}`);
engine.setCrossOut(0, 0, null);
// cleared: the same images, nothing written
const keptLevel = Uint8Array.from(level.bytes), keptCross = Uint8Array.from(cross.bytes);
const wire2 = new Uint8Array(wire.length), offsets2 = new Float64Array(S + 1);
engine.computeColumnsPcmPacked(src, sources, frames, format, fftSize, hop, true, wire2, offsets2);
for (let i = 0; i < keptLevel.length; i++) if (level.bytes[i] !== keptLevel[i]) throw new Error('cleared level records were written');
for (let i = 0; i < keptCross.length; i++) if (cross.bytes[i] !== keptCross[i]) throw new Error('cleared cross records were written');
for (let s = 0; s <= S; s++) if (offsets[s] !== offsets2[s]) throw new Error('offsets differ with and without the level meters');
for (let i = 0; i < offsets[S]; i++) if (wire[i] !== wire2[i]) throw new Error(`the wire images differ at ${i} with and without the level meters`);
engine.destroy();

// the host forms on float streams of their own
const L = 1024 + 255 * 9 + 100, pcm = new Float32Array(4 * L);
for (let i = 0; i < pcm.length; i++) pcm[i] = Math.fround(Math.sin(i * 0.37) * ((i * 7919) % 13) / 8);
pcm[500] = NaN; pcm[600] = -0; pcm[601] = 1e-40; pcm[L + 700] = Infinity; pcm[2 * L + 900] = -300;
const levelsOf = em.levelsOf(pcm, 4, L, 1024, 255, 4), crossOf = em.crossOf(pcm, 2, 2, 1, 0, L, 1024, 255, 4);

fs.writeFileSync(path.join(outDir, 'src.i16'), Buffer.from(src.buffer));
fs.writeFileSync(path.join(outDir, 'level.bin'), Buffer.from(level.bytes.buffer, 0, S * Jr * 24));
fs.writeFileSync(path.join(outDir, 'cross.bin'), Buffer.from(cross.bytes.buffer, 0, sources * Jr * 16));
fs.writeFileSync(path.join(outDir, 'pcm.f32'), Buffer.from(pcm.buffer));
fs.writeFileSync(path.join(outDir, 'levels_of.bin'), Buffer.from(levelsOf.bytes.buffer));
fs.writeFileSync(path.join(outDir, 'cross_of.bin'), Buffer.from(crossOf.bytes.buffer));
console.log(JSON.stringify({ sources, views: format.views, frames, fftSize, hop, factor, columns: J, mix: Array.from(format.mix), L }));
