// The live calls' overlays through the addon (engine.setLivePeaks / engine.setLiveWave), for tests/test_gpu_live_overlay_node.py:
// 64 streams x 20 hops of N = 4096 / hop 256, one computeSpectrogramColumns call per hop, then the flushes.  After every call
// engine.columnsPeaks must be peaksOf(engine.columnsDb) and engine.columnsWave the pair waveOf gives for the column the call
// emitted ((+inf, -inf) for the empty column), bit for bit.  Prints one JSON line.
'use strict';
const em = require('./index.js');

const S = 64, fftSize = 4096, hop = 256, hops = 20, k = 8, minDb = -60;
const L = fftSize + hop * (hops - 1);
const pcm = new Float32Array(S * L);
for (let s = 0; s < S; s++)
  for (let i = 0; i < L; i++)
    pcm[s * L + i] = Math.fround(0.4 * Math.sin(2 * Math.PI * (110 + 37 * s) * i / 48000) + 0.2 * Math.sin(2 * Math.PI * (2000 + 91 * s) * i / 48000 + s) +
      (i % (700 + s) === 0 ? 0.3 : 0));
pcm[3 * L + 2500] = NaN; pcm[4 * L + 2600] = -Infinity; pcm[5 * L + 2700] = -0;

const bits = (a) => new Uint32Array(a.buffer, a.byteOffset, a.length);
function sameBits(a, b, what) {
  const x = bits(a), y = bits(b);
  if (x.length !== y.length) throw new Error(`${what}: ${x.length} values against ${y.length}`);
  for (let i = 0; i < x.length; i++) if (x[i] !== y[i]) throw new Error(`${what}: differs at ${i}: ${a[i]} against ${b[i]}`);
}

const engine = em.createEngine({ streams: S });
const R = engine.rows;
engine.setLivePeaks({ k, minDb });
engine.setLiveWave(true);
if (engine.columnsPeaks.length !== S * k * 2 || engine.columnsWave.length !== S * 2) throw new Error('overlay blocks are not sized like columnsDb');
const want = em.waveOf(pcm, S, L, fftSize, hop, 1);          // [S][hops] pairs
const frames = new Float32Array(S * fftSize);
let emitted = 0, empty = 0, withPeaks = 0;

function check(call) {
  const db = engine.columnsDb;
  sameBits(engine.columnsPeaks, em.peaksOf(db, S, R, k, minDb), `${call}: peaks`);
  const pair = new Float32Array(2);
  for (let s = 0; s < S; s++) {
    const c = engine.columnIndex[s];
    if (c < 0) { pair[0] = Infinity; pair[1] = -Infinity; empty++; } else { pair[0] = want[(s * hops + c) * 2]; pair[1] = want[(s * hops + c) * 2 + 1]; emitted++; }
    sameBits(engine.columnsWave.subarray(2 * s, 2 * s + 2), pair, `${call}: envelope of stream ${s}, column ${c}`);
    if (engine.columnsPeaks[s * k * 2] >= 0) withPeaks++;
  }
}
for (let j = 0; j < hops; j++) {
  for (let s = 0; s < S; s++) frames.set(pcm.subarray(s * L + j * hop, s * L + j * hop + fftSize), s * fftSize);
  engine.computeSpectrogramColumns(frames, fftSize, hop, true);
  check(`hop ${j}`);
}
const D = em.latencyColumns(fftSize, hop, true);
for (let i = 0; i < D; i++) { engine.flushColumns(); check(`flush ${i}`); }
if (emitted !== S * hops || empty !== S * D || withPeaks === 0) throw new Error(`emitted ${emitted}, empty ${empty}, with peaks ${withPeaks}`);

// mid-session the envelope cannot be switched on again; cleared, the calls leave the blocks alone
engine.setLiveWave(false);
engine.setLivePeaks(null);
if (engine.columnsPeaks !== undefined || engine.columnsWave !== undefined) throw new Error('cleared overlays keep their blocks');
let code = 'none';
try { engine.setLiveWave(true); } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_STATE') throw new Error(`setLiveWave mid-session gave ${code}`);
try { engine.setLivePeaks({ k: 33 }); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`k = 33 gave ${code}`);
engine.reset();
engine.setLiveWave(true);
engine.destroy();
console.log(JSON.stringify({ ok: true, S, hops, k, emitted, empty, withPeaks }));
