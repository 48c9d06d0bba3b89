// The waveform envelope through the addon (engine.setWaveOut with engine.computeColumnsPcmPacked, waveOf), for
// tests/test_gpu_wave.py: writes the raw input and the bytes it got to the directory in argv[2]; the test makes the same calls
// through the ctypes binding and compares.  EXACT engine: the wire images are reproducible (the envelope is in either mode).
'use strict';
const fs = require('fs');
const path = require('path');
const em = require('./index.js');

const outDir = process.argv[2];
const sources = 2, fftSize = 4096, hop = 256, factor = 3;
const frames = fftSize + hop * 59 + 3;
const format = em.pcmFormat({ type: 's16', channels: 2, views: ['left', 'right', 'mid', 'side'] });
const S = sources * format.views;
const src = new Int16Array(sources * frames * 2);
for (let s = 0; s < sources; s++)
  for (let i = 0; i < frames; i++) {
    src[(s * frames + i) * 2] = Math.round(9000 * Math.sin(2 * Math.PI * (110 + 60 * s) * i / 48000) + 3000 * Math.sin(2 * Math.PI * 2345.6 * i / 48000));
    src[(s * frames + i) * 2 + 1] = Math.round(7000 * Math.sin(2 * Math.PI * (331 + 40 * s) * i / 48000 + 1) + (i % 9000 === 0 ? 12000 : 0));
  }

const engine = em.createEngine({ exact: true, streams: S, timeReduce: factor });
const R = engine.rows, J = em.numColumns(frames, fftSize, hop), Jr = Math.ceil(J / factor);
const wire = new Uint8Array(S * em.wireBound(Jr, R)), offsets = new Float64Array(S + 1);
const wave = new Float32Array(S * Jr * 2 + 2).fill(7);   // (one pair more than needed: it stays as it is)
engine.setWaveOut(wave);
engine.computeColumnsPcmPacked(src, sources, frames, format, fftSize, hop, true, wire, offsets);
if (wave[S * Jr * 2] !== 7 || wave[S * Jr * 2 + 1] !== 7) throw new Error('the envelope was written past streams x columns pairs');
// one pair short: refused before anything runs, and the engine stays usable
let code;
engine.setWaveOut(new Float32Array(S * Jr * 2 - 2));
try { engine.computeColumnsPcmPacked(src, sources, frames, format, fftSize, hop, true, wire, offsets); } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`an envelope one pair short gave ${code}`);
try { engine.setWaveOut(new Uint8Array(16)); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`a Uint8Array envelope gave ${code}`);
// cleared: the same images, nothing written
engine.setWaveOut(null);
const kept = Float32Array.from(wave);
const wire2 = new Uint8Array(wire.length), offsets2 = new Float64Array(S + 1);
engine.computeColumnsPcmPacked(src, sources, frames, format, fftSize, hop, true, wire2, offsets2);
for (let i = 0; i < wave.length; i++) if (!Object.is(wave[i], kept[i])) throw new Error('a cleared envelope was written');
for (let s = 0; s <= S; s++) if (offsets[s] !== offsets2[s]) throw new Error('offsets differ with and without the envelope');
for (let i = 0; i < offsets[S]; i++) if (wire[i] !== wire2[i]) throw new Error(`the wire images differ at ${i} with and without the envelope`);
engine.destroy();

// the host twin on float streams of its own
const L = 1024 + 255 * 9 + 100, pcm = new Float32Array(3 * L);
for (let i = 0; i < pcm.length; i++) pcm[i] = Math.fround(Math.sin(i * 0.37) * ((i * 7919) % 13));
pcm[5] = NaN; pcm[600] = -0; pcm[601] = 0; pcm[L + 700] = Infinity;
const waveOf = em.waveOf(pcm, 3, L, 1024, 255, 4);

fs.writeFileSync(path.join(outDir, 'src.i16'), Buffer.from(src.buffer));
fs.writeFileSync(path.join(outDir, 'wire.u8'), Buffer.from(wire.buffer, 0, offsets[S]));
fs.writeFileSync(path.join(outDir, 'wave.f32'), Buffer.from(wave.buffer, 0, S * Jr * 8));
fs.writeFileSync(path.join(outDir, 'pcm.f32'), Buffer.from(pcm.buffer));
fs.writeFileSync(path.join(outDir, 'wave_of.f32'), Buffer.from(waveOf.buffer));
console.log(JSON.stringify({ sources, views: format.views, frames, fftSize, hop, factor, columns: J, rows: R, offsets: Array.from(offsets),
  mix: Array.from(format.mix), L }));
