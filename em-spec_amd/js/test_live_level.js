// The live level meters through the addon (engine.setLiveLevel / engine.setLiveCross, em.levelSum / em.crossSum), for
// tests/test_gpu_live_level_node.py: 8 streams = 4 pairs x 20 hops of N = 4096 / hop 256, one computeSpectrogramColumns call per
// hop, then the flushes.  After every call engine.columnsLevel must hold the record levelsOf gives for the column each stream
// emitted and engine.columnsCross the record crossOf gives for each pair (all zero for the empty column), byte for byte; the
// summed records of the pair whose second stream is the inverted first give a correlation of exactly -1.  Prints one JSON line.
'use strict';
const em = require('./index.js');

const S = 8, views = 2, pairs = S / views, fftSize = 4096, hop = 256, hops = 20;
const L = fftSize + hop * (hops - 1);
const pcm = new Float32Array(S * L);
for (let s = 0; s < S; s++)
  for (let i = 0; i < L; i++)
    pcm[s * L + i] = Math.fround(0.4 * Math.sin(2 * Math.PI * (110 + 37 * s) * i / 48000) + 0.2 * Math.sin(2 * Math.PI * (2000 + 91 * s) * i / 48000 + s) +
      (i % (700 + s) === 0 ? 0.3 : 0));
for (let i = 0; i < L; i++) pcm[1 * L + i] = -pcm[i];            // pair 0: the inverted copy
pcm[2 * L + 2500] = NaN; pcm[3 * L + 2600] = -Infinity; pcm[4 * L + 2700] = 200; pcm[5 * L + 2800] = -0;

function sameBytes(a, b, what) {
  if (a.length !== b.length) throw new Error(`${what}: ${a.length} bytes against ${b.length}`);
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(`${what}: differs at byte ${i}: ${a[i]} against ${b[i]}`);
}

const engine = em.createEngine({ streams: S });
engine.setLiveLevel(true);
engine.setLiveCross(views, 0, 1);
if (engine.columnsLevel.count !== S || engine.columnsCross.count !== pairs) throw new Error('record blocks are not sized for one column per stream');
const wantLevel = em.levelsOf(pcm, S, L, fftSize, hop, 1);                  // [S][hops]
const wantCross = em.crossOf(pcm, pairs, views, 0, 1, L, fftSize, hop, 1);  // [pairs][hops]
const frames = new Float32Array(S * fftSize);
const keptLevel = em.levelRecords(2 * hops), keptCross = em.crossRecords(hops);   // pair 0's emitted records, column by column
let emitted = 0, empty = 0, odd = 0;

function check(call) {
  for (let s = 0; s < S; s++) {
    const c = engine.columnIndex[s];
    const got = engine.columnsLevel.bytes.subarray(24 * s, 24 * s + 24);
    const want = c < 0 ? new Uint8Array(24) : wantLevel.bytes.subarray(24 * (s * hops + c), 24 * (s * hops + c) + 24);
    sameBytes(got, want, `${call}: level of stream ${s}, column ${c}`);
    if (c < 0) empty++; else emitted++;
    odd += engine.columnsLevel.words[6 * s + 5];
    if (s < 2 && c >= 0) keptLevel.bytes.set(got, 24 * (s * hops + c));
  }
  for (let p = 0; p < pairs; p++) {
    const c = engine.columnIndex[p * views];
    const got = engine.columnsCross.bytes.subarray(16 * p, 16 * p + 16);
    const want = c < 0 ? new Uint8Array(16) : wantCross.bytes.subarray(16 * (p * hops + c), 16 * (p * hops + c) + 16);
    sameBytes(got, want, `${call}: cross of pair ${p}, column ${c}`);
    if (p === 0 && c >= 0) keptCross.bytes.set(got, 16 * c);
  }
}
for (let j = 0; j < hops; j++) {
  for (let s = 0; s < S; s++) frames.set(pcm.subarray(s * L + j * hop, s * L + j * hop + fftSize), s * fftSize);
  engine.computeSpectrogramColumns(frames, fftSize, hop, true);
  check(`hop ${j}`);
}
const D = em.latencyColumns(fftSize, hop, true);
for (let i = 0; i < D; i++) { engine.flushColumns(); check(`flush ${i}`); }
if (emitted !== S * hops || empty !== S * D || odd < 3) throw new Error(`emitted ${emitted}, empty ${empty}, odd ${odd}`);

// the meter's integration: all 20 hops of pair 0 as one record each
const la = em.levelSum(keptLevel, 0, hops), lb = em.levelSum(keptLevel, hops, hops), ab = em.crossSum(keptCross);
sameBytes(la.bytes, em.levelsOf(pcm.subarray(0, L), 1, L, fftSize, hop, hops).bytes, 'levelSum against the factor-20 record');
sameBytes(ab.bytes, em.crossOf(pcm.subarray(0, 2 * L), 1, 2, 0, 1, L, fftSize, hop, hops).bytes, 'crossSum against the factor-20 record');
const rho = em.crossCorrelation(la, 0, lb, 0, ab, 0);
if (rho !== -1) throw new Error(`the inverted pair's correlation is ${rho}`);
const { rmsDb } = em.levelValues(la, 0, hops * hop);
if (!(rmsDb < 0 && rmsDb > -20)) throw new Error(`rms ${rmsDb} dB`);
let code = 'none';
try { em.levelSum(keptLevel, 0, 0); } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`levelSum of no record gave ${code}`);

// mid-session the meters cannot be switched on again; a stream of a pair cannot restart alone; cleared, the blocks are gone
engine.setLiveLevel(null);
try { engine.setLiveLevel(true); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_STATE') throw new Error(`setLiveLevel mid-session gave ${code}`);
try { engine.resetStream(1); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_STATE') throw new Error(`resetStream with a live cross set gave ${code}`);
engine.setLiveCross(null);
if (engine.columnsLevel !== undefined || engine.columnsCross !== undefined) throw new Error('cleared meters keep their blocks');
engine.resetStream(1);
try { engine.setLiveCross(65, 0, 1); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`views = 65 gave ${code}`);
engine.reset();
engine.setLiveLevel(true);
engine.destroy();
console.log(JSON.stringify({ ok: true, S, pairs, hops, emitted, empty, odd, rho }));
