// The live history through the addon (engine.setLiveHistory / liveHistory / historyView), for tests/test_gpu_live_history_node.py:
//   node test_history.js <feed.f32> <out.bin> S L fftSize hop rows W
// feed: float32 [S][L].  One EXACT session: one computeSpectrogramColumns call per hop, then the flushes; after every call
// liveHistory must give the columns emitted so far and the first one held.  Then the views listed below, their dB, index and
// RGBA bytes appended to out.bin in order - the Python test makes the same feed through its own binding and compares the bytes.
// Prints one JSON line.
'use strict';
const fs = require('fs');
const em = require('./index.js');

const [feedPath, outPath] = process.argv.slice(2, 4);
const [S, L, fftSize, hop, rows, W] = process.argv.slice(4, 10).map(Number);
const raw = fs.readFileSync(feedPath);
const pcm = new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4);
if (pcm.length !== S * L) throw new Error(`feed holds ${pcm.length} samples, not ${S * L}`);

const engine = em.createEngine({ streams: S, rows, exact: true });
if (engine.liveHistory(0) !== null) throw new Error('a history before it is set');
engine.setLiveHistory(W);
const hops = (L - fftSize) / hop + 1, D = em.latencyColumns(fftSize, hop, true);
const frames = new Float32Array(S * fftSize);
let emitted = 0;
function held(call) {
  for (let s = 0; s < S; s++) {
    const h = engine.liveHistory(s);
    if (!h || h.end !== emitted || h.first !== Math.max(0, emitted - W)) throw new Error(`${call}: stream ${s} holds ${JSON.stringify(h)}, emitted ${emitted}`);
  }
}
for (let j = 0; j < hops; j++) {
  for (let s = 0; s < S; s++) frames.set(pcm.subarray(s * L + j * hop, s * L + j * hop + fftSize), s * fftSize);
  engine.computeSpectrogramColumns(frames, fftSize, hop, true);
  if (engine.columnIndex[0] >= 0) emitted++;
  held(`hop ${j}`);
}
for (let i = 0; i < D; i++) { engine.flushColumns(); emitted++; held(`flush ${i}`); }

const map = { dbTop: -6, dbRange: 55, gateDb: -58.5, shiftDb: 4.25 };
const first = emitted - W;
const views = [
  { firstColumn: first, factor: 1, groups: W, want: ['db', 'index', 'rgba'] },
  { firstColumn: first, factor: 2, groups: Math.ceil(W / 2), map, want: ['db', 'index', 'rgba'] },
  { firstColumn: first + 1, factor: 3, groups: Math.ceil((W - 1) / 3), stream0: 1, streams: S - 1, map, want: ['db', 'index', 'rgba'] },
  { firstColumn: first, factor: 65536, groups: 1, want: ['db', 'index', 'rgba'] },
];
const chunks = [];
for (const v of views) {
  const o = engine.historyView(v);
  for (const a of [o.db, o.index, o.rgba]) chunks.push(Buffer.from(a.buffer, a.byteOffset, a.byteLength));
}
fs.writeFileSync(outPath, Buffer.concat(chunks));

// refusals leave the engine usable
let code = 'none';
try { engine.historyView({ firstColumn: first - 1, groups: 1 }); } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_INVALID_ARG') throw new Error(`a view below the held range gave ${code}`);
try { engine.setLiveHistory(W); code = 'none'; } catch (e) { code = e.code; }
if (code !== 'EMSPEC_ERR_STATE') throw new Error(`setLiveHistory mid-session gave ${code}`);
if (engine.historyView({ firstColumn: first, groups: 1 }).db.length !== S * rows) throw new Error('a view after the refusals');
engine.setLiveHistory(0);
if (engine.liveHistory(0) !== null) throw new Error('a cleared history still answers');
engine.destroy();
console.log(JSON.stringify({ ok: true, S, hops, W, emitted, views: views.length, first }));
