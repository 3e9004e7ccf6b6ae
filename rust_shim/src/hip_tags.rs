//! Row-tag codes for the tagged searches of libcqs_hip.so (include/cqs_hip.h, "row tags"): what the dense shim
//! (`hip.rs`) and the sparse one (`hip_splade_index.rs`) share.  Pure Rust, no FFI.
//!
//! Drop-in location: `src/hip_tags.rs`, `#[cfg(any(feature = "hip-index", feature = "hip-aux"))] pub mod hip_tags;`.
//!
//! The predicate `search_hybrid_inner` builds for both legs of every hybrid query (src/search/query.rs:860-877) is
//! "chunk type in an include set, not in an exclude set, language in a set; a chunk without metadata never passes": a
//! function of two small integers per chunk.  `TagCodes` assigns those integers from `chunk_type_language_map` when an
//! index is opened; the library keeps them beside the rows in HBM, and a filtered search sends 128 bytes of allowed
//! sets instead of calling the predicate once per chunk and uploading n / 8 bytes.
//!
//! Tag layout (the library gives the four 8-bit fields no meaning; this is the shim's use of them): field 0 = chunk-type
//! code, field 1 = language code, code 255 = "no metadata", fields 2 and 3 spare (0, never constrained).

use std::collections::HashMap;

use crate::parser::{ChunkType, Language};

/// Code of a chunk that `chunk_type_language_map` does not know: it passes only the filter that constrains nothing.
pub const NO_META: u32 = 255;
/// The filter: four 256-bit sets, bit v of field f's set = bit v % 32 of word 8 f + v / 32.
pub type Allow = [u32; 32];

pub struct TagCodes {
    types: HashMap<ChunkType, u32>,
    langs: HashMap<Language, u32>,
}

impl TagCodes {
    /// Codes 0, 1, .. in first-seen order.  `None` when a field would need more than 255 codes (code 255 is taken):
    /// the caller keeps the host-bitset path.
    pub fn assign(meta: &HashMap<String, (ChunkType, Language)>) -> Option<Self> {
        let mut codes = TagCodes { types: HashMap::new(), langs: HashMap::new() };
        for (ct, lang) in meta.values() {
            let next = codes.types.len() as u32;
            codes.types.entry(*ct).or_insert(next);
            let next = codes.langs.len() as u32;
            codes.langs.entry(*lang).or_insert(next);
            if codes.types.len() > NO_META as usize || codes.langs.len() > NO_META as usize {
                return None;
            }
        }
        Some(codes)
    }

    /// The tag of one chunk id.
    pub fn tag_of(&self, id: &str, meta: &HashMap<String, (ChunkType, Language)>) -> u32 {
        match meta.get(id) {
            Some((ct, lang)) => self.types[ct] | (self.langs[lang] << 8),
            None => NO_META | (NO_META << 8),
        }
    }

    /// The reference's predicate as allowed sets: field 0 = include types (or all) minus exclude types, field 1 =
    /// languages (or all); bit 255 of field 0 is cleared as soon as any of the three is `Some` (a chunk without metadata
    /// never passes then); with none of them `Some` every bit is set.  A type or language no chunk has owns no code and
    /// adds nothing to its set.
    pub fn allow(&self, include: Option<&[ChunkType]>, exclude: Option<&[ChunkType]>, languages: Option<&[Language]>) -> Allow {
        let mut allow: Allow = [u32::MAX; 32];
        if include.is_none() && exclude.is_none() && languages.is_none() {
            return allow;
        }
        let mut set = |allow: &mut Allow, field: usize, code: u32, on: bool| {
            let (w, bit) = (8 * field + (code / 32) as usize, 1u32 << (code % 32));
            if on { allow[w] |= bit } else { allow[w] &= !bit }
        };
        if let Some(types) = include {
            allow[0..8].fill(0);
            for ct in types {
                if let Some(&c) = self.types.get(ct) {
                    set(&mut allow, 0, c, true);
                }
            }
        }
        if let Some(types) = exclude {
            for ct in types {
                if let Some(&c) = self.types.get(ct) {
                    set(&mut allow, 0, c, false);
                }
            }
        }
        if let Some(langs) = languages {
            allow[8..16].fill(0);
            for lang in langs {
                if let Some(&c) = self.langs.get(lang) {
                    set(&mut allow, 1, c, true);
                }
            }
        }
        set(&mut allow, 0, NO_META, false);
        allow
    }
}
