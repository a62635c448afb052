"""utils: part of the MI355X-native DH-AUG package."""
